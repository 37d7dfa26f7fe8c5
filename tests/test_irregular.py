"""Irregular device profiles and head placements on the CPU (tests/irregular_cases.py): the case list reaches
every flag bit, device class and head placement the device code branches on; the C packer, the host lowering,
the fleet constants, HiGHS, the NumPy plan evaluation and the exact oracle agree on it; both oracle solvers
reproduce the reference's recorded results (tests/golden/irregular.json). No GPU."""

import numpy as np
import pytest

from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import F64_FIELDS, BYTE_FIELDS, fleet_table, fleet_table_py
from distilp_amd.solver.lower import lower_fleet
from oracle import milp_oracle as mo

from . import irregular_cases as ic
from . import pressure_cases as pc
from .conftest import load_json
from .test_lowering import _check

HEAD, UMA, CPU_RATE, GPU, GPU_RATE, CUDA_OK, METAL_OK, METAL_AVAIL = (1 << b for b in range(8))


def by_model(case_list):
    """{model id: (model, [cases])}: the cases of a list grouped by the model they run on."""
    out = {}
    for c in case_list:
        out.setdefault(id(ic.model_of(c)), (ic.model_of(c), []))[1].append(c)
    return list(out.values())


# ------------------------------------------------------------------ structure
def test_case_list_structure():
    """Conditions on the committed case list (not measurements); the oracle alone meets them. Measured: 193
    instances, all supported and feasible, 157 unique (81 %), 126 with a positive slack or t (65 %)."""
    names = {e for c in ic.CASES for e in c[4]}
    assert names == set(ic.EDIT_NAMES), set(ic.EDIT_NAMES) ^ names
    # every device / head edit changed a field of the device it names; a model edit changed the model
    for c in ic.CASES:
        M, scale, seed, _, edits = c
        ds = [dict(d) for d in pc.pressured_fleet(seed, M, scale)]
        for name in edits:
            if name in ic.MODEL_EDITS:
                field = "f_q" if name == "f_q_no_b1" else "f_out"
                assert "b_1" in getattr(pc.our_model(), field) and "b_1" not in getattr(ic.model_of(c), field)
                continue
            before = [repr(sorted(d.items())) for d in ds]
            idx = ic.apply_edit(ds, name)
            after = [repr(sorted(d.items())) for d in ds]
            changed = [i for i in range(M) if before[i] != after[i]]
            assert changed, (c, name, "no-op")
            assert set(changed) <= set(idx) | ({0} if ic.is_head_edit(name) else set()), (c, name, changed, idx)
            if not ic.is_head_edit(name) and name != "slow_disk_head":
                assert min(idx) > 0, (c, name)
    # shapes, scales and kv widths
    for M in (2, 3, 5, 16, 33):
        assert {c[1] for c in ic.cases(Ms=(M,))} == {ic.ONE, ic.S16}, M
    assert {c[0] for c in ic.CASES} == {2, 3, 5, 16, 33, 64, 70, 100}
    n16 = sum(c[3] == "fp16" for c in ic.CASES)
    assert 0.25 * len(ic.CASES) <= n16 <= 0.35 * len(ic.CASES), n16  # a quarter (13 of 49)
    heads64 = {ic.touched(c)[e][0] for c in ic.cases(Ms=(64,)) for e in c[4] if e.startswith("head_at:")}
    assert {1, 31, 32, 63} <= heads64
    assert any("head_at:66" in c[4] for c in ic.cases(Ms=(70,))) and any("no_head" in c[4] for c in ic.cases(Ms=(70,)))
    # the shape whose tables exceed the LDS budget: a head in the second 64-device chunk, and none
    assert any("head_at:last" in c[4] for c in ic.cases(Ms=(100,))) and any("no_head" in c[4] for c in ic.cases(Ms=(100,)))
    for M in (2, 3, 5, 16, 33, 64, 70, 100):  # a head edit with three or more device edits
        assert any(sum(ic.is_head_edit(e) for e in c[4]) >= 1 and sum(e in ic.DEVICE_EDITS for e in c[4]) >= 3
                   for c in ic.cases(Ms=(M,))), M
    combo = [c for c in ic.cases(Ms=(16,)) if {"cuda_and_metal", "head_at:linux_cuda", "cuda_uma"} <= set(c[4])]
    assert combo and len({i for v in ic.touched(combo[0]).values() for i in v}) == 1

    # the packed table of the whole list
    flags, cls, per_fleet = [], [], []
    for model, cs in by_model(ic.CASES):
        t = fleet_table([ic.devices(c) for c in cs], model)
        flags.append(t.flags.copy())
        cls.append(t.os_class.copy())
        per_fleet += [t.flags[t.dev_off[f]:t.dev_off[f + 1]] for f in range(t.n_fleets)]
    flags, cls = np.concatenate(flags), np.concatenate(cls)
    for bit in range(8):
        assert (flags & (1 << bit)).any() and (~flags & (1 << bit)).any(), bit
    for s in (1, 2, 3):
        assert ((cls == s) & (flags & HEAD != 0)).any() and ((cls == s) & (flags & HEAD == 0)).any(), s
    both = (flags & CUDA_OK != 0) & (flags & METAL_OK != 0)
    assert both.any()
    n_heads = [int((f & HEAD != 0).sum()) for f in per_fleet]
    assert 0 in n_heads and max(n_heads) > 1
    # combinations the five clean kinds never give
    assert ((flags & CUDA_OK != 0) & (flags & GPU == 0)).any()          # cuda_no_rate / cuda_no_load
    assert ((flags & GPU != 0) & (flags & (CUDA_OK | METAL_OK) == 0)).any()  # cuda_no_vram / metal_none
    assert ((cls == 1) & (flags & CUDA_OK != 0)).any()                    # m1_with_gpu
    assert ((cls == 2) & (flags & METAL_AVAIL != 0) & (flags & METAL_OK == 0)).any()  # metal_off

    sh = ic.shares()
    print("irregular:", sh, "two-row devices:", int(both.sum()))
    assert 150 <= sh["instances"] <= 250, sh
    assert sh["supported"] == sh["instances"], sh
    assert sh["feasible"] >= 0.90 * sh["instances"], sh
    assert sh["unique"] >= 0.75 * sh["feasible"], sh
    assert sh["slack_or_t"] >= 0.25 * sh["feasible"], sh


# ------------------------------------------------------------------ the packer
def test_c_packer_equals_the_python_packer():
    for model, cs in by_model(ic.CASES):
        fleets = [ic.devices(c) for c in cs]
        a, b = fleet_table(fleets, model), fleet_table_py(fleets, model)
        assert hasattr(a, "_heads")  # the C packer's table
        for f in ("dev_off", "os_class", "flags") + tuple(F64_FIELDS) + tuple(BYTE_FIELDS):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
            assert getattr(a, f).dtype == getattr(b, f).dtype, f
        want = [int(t.dev_off[f]) + next((i for i, d in enumerate(devs) if d.is_head), 0)
                for t in (a,) for f, devs in enumerate(fleets)]
        assert a._heads.tolist() == want


# One hand-checked fleet per edit: pressured_fleet(6, 5, 1) = [mac_metal head, linux_cpu, linux_cuda, mac_metal,
# android] (B6), or pressured_fleet(4, 5, 1) = [mac_metal head, linux_cpu, android, mac_no_metal, android] (B4).
# The bits: HEAD 1, UMA 2, CPU_RATE 4, GPU 8, GPU_RATE 16, CUDA_OK 32, METAL_OK 64, METAL_AVAIL 128.
#   mac_metal      UMA | CPU_RATE | GPU | GPU_RATE | METAL_OK | METAL_AVAIL = 222 (223 as the head), class 2
#   linux_cuda     CPU_RATE | GPU | GPU_RATE | CUDA_OK = 60, class 3
#   linux_cpu, android   CPU_RATE = 4, class 3;   mac_no_metal   UMA | CPU_RATE = 6, class 1
B6_FLAGS, B6_CLS = [223, 4, 60, 222, 4], [2, 3, 3, 2, 3]
B4_FLAGS, B4_CLS = [223, 4, 4, 6, 4], [2, 3, 3, 1, 3]
EXPECTED = {  # edit: (seed, flags, os_class)
    "no_head": (6, [222, 4, 60, 222, 4], B6_CLS),
    "head_at:1": (6, [222, 5, 60, 222, 4], B6_CLS),
    "head_at:last": (6, [222, 4, 60, 222, 5], B6_CLS),
    "head_at:linux_cuda": (6, [222, 4, 61, 222, 4], B6_CLS),
    "head_at:android": (6, [222, 4, 60, 222, 5], B6_CLS),
    "head_at:mac_no_metal": (4, [222, 4, 4, 7, 4], B4_CLS),
    "two_heads": (6, [223, 4, 60, 222, 5], B6_CLS),
    "all_heads": (6, [223, 5, 61, 223, 5], B6_CLS),
    # d_avail_metal None: the GPU table and load stay (GPU, GPU_RATE); neither Metal row
    "metal_none": (6, [223, 4, 60, 2 + 4 + 8 + 16, 4], B6_CLS),
    # has_metal False: no GPU table; d_avail_metal is still there (the M2 RAM row)
    "metal_off": (6, [223, 4, 60, 2 + 4 + 128, 4], B6_CLS),
    "cuda_and_metal": (6, [223, 4, 60 + 64 + 128, 222, 4], B6_CLS),
    "cuda_no_rate": (6, [223, 4, 4 + 32, 222, 4], B6_CLS),
    "cuda_no_load": (6, [223, 4, 4 + 32, 222, 4], B6_CLS),
    "cuda_no_vram": (6, [223, 4, 4 + 8 + 16, 222, 4], B6_CLS),
    "cuda_uma": (6, [223, 4, 62, 222, 4], B6_CLS),
    "scpu_no_q": (6, [223, 0, 60, 222, 4], B6_CLS),
    "sgpu_no_q": (6, [223, 4, 4 + 8 + 32, 222, 4], B6_CLS),
    "scpu_zero": (6, B6_FLAGS, B6_CLS),
    "android_swap": (6, B6_FLAGS, B6_CLS),
    "android_swap_rev": (6, B6_FLAGS, B6_CLS),
    "slow_disk": (6, B6_FLAGS, B6_CLS),
    "slow_disk_head": (6, B6_FLAGS, B6_CLS),
    "slow_gpu": (6, B6_FLAGS, B6_CLS),
    "kvcpy": (6, B6_FLAGS, B6_CLS),
    "m1_with_gpu": (6, B6_FLAGS, [2, 3, 1, 2, 3]),
    "cgpu_over": (6, B6_FLAGS, B6_CLS),
    "f_q_no_b1": (6, B6_FLAGS, B6_CLS),
    "f_out_no_b1": (6, B6_FLAGS, B6_CLS),
}
# the value fields an edit that leaves the flags alone must show: edit -> (field, device, value)
EXPECTED_FIELDS = {
    "scpu_zero": ("scpu_b1", 1, 0.0), "android_swap": ("swap", 4, float(1 << 30)),
    "android_swap_rev": ("swap", 4, float(1 << 30)), "slow_disk": ("s_disk", 1, 0.5),
    "slow_disk_head": ("s_disk", 0, 0.5), "slow_gpu": ("t_kvcpy_gpu", 2, 0.01), "kvcpy": ("t_kvcpy_cpu", 2, 0.002),
}


def test_flag_bytes_equal_the_hand_checked_tables():
    from distilp_amd.common import DeviceProfile

    assert set(EXPECTED) == {e for e in ic.EDIT_NAMES if e.split(":")[-1] not in ("31", "32", "63", "66")}
    base = fleet_table([[DeviceProfile.model_validate(d) for d in pc.pressured_fleet(6, 5, ic.ONE)]], pc.our_model())
    assert (base.flags.tolist(), base.os_class.tolist()) == (B6_FLAGS, B6_CLS)
    base4 = fleet_table([[DeviceProfile.model_validate(d) for d in pc.pressured_fleet(4, 5, ic.ONE)]], pc.our_model())
    assert (base4.flags.tolist(), base4.os_class.tolist()) == (B4_FLAGS, B4_CLS)
    for name, (seed, flags, cls) in EXPECTED.items():
        case = (5, ic.ONE, seed, "4bit", (name,))
        for pack in (fleet_table, fleet_table_py):
            t = pack([ic.devices(case)], ic.model_of(case))
            assert (t.flags.tolist(), t.os_class.tolist()) == (flags, cls), (name, pack.__name__, t.flags.tolist())
            if name in EXPECTED_FIELDS:
                field, i, v = EXPECTED_FIELDS[name]
                assert getattr(t, field)[i] == v and getattr(base, field)[i] != v, (name, field)
        if name == "slow_gpu":
            assert t.T_gpu[2] == t.T_cpu[2] / 50
        if name == "cgpu_over":
            assert t.c_gpu[2] == t.d_avail_cuda[2] + (1 << 30)
        if name == "cuda_and_metal":
            assert t.d_avail_metal[2] == t.d_avail_cuda[2] // 2 and t.T_gpu[2] == base.T_gpu[0]  # the Metal load wins
            assert t.sgpu_b1[2] == base.sgpu_b1[0] != base.sgpu_b1[2]                        # and the Metal table
    for j, M, seed in ((31, 64, 1), (32, 64, 2), (63, 64, 3), (66, 70, 1)):  # the lanes of the wide fleets
        case = (M, ic.S16, seed, "4bit", (f"head_at:{j}",))
        t = fleet_table([ic.devices(case)], ic.model_of(case))
        assert np.flatnonzero(t.flags & HEAD).tolist() == [j] and t._heads.tolist() == [j]


# ------------------------------------------------------------------ the host lowering
def test_host_lowering_and_constants_equal_the_oracle():
    from distilp_amd.solver.coefficients import assign_sets
    from distilp_amd.solver.fleets import fleet_constants, fleet_constants_np
    from distilp_amd.solver.halda import _offset_parts

    rows2 = 0
    for c in ic.CASES:
        devs, model = ic.devices(c), ic.model_of(c)
        fl = lower_fleet(devs, model, c[3])
        for k in ic.ks_of(c[0]):
            p = ic.problem(c, k)
            _check(fl, k, p)
            assert fl.obj_offset_parts == tuple(p["const"]), (c, k)
        sets = assign_sets(devs)
        assert sets == mo.sets_of(devs)
        want = _offset_parts(devs, model, sets)
        assert want == tuple(ic.problem(c, 1)["const"]), c
        t = fleet_table([devs], model)
        assert tuple(v[0] for v in fleet_constants(t, model)) == want, c
        assert tuple(v[0] for v in fleet_constants_np(t, model)) == want, c
        assert t.sets(0) == sets
        rows2 += int(((t.flags & CUDA_OK != 0) & (t.flags & METAL_OK != 0)).sum())
    assert rows2 >= 8


# ------------------------------------------------------------------ reference behaviour
def _highs_agrees(case, k, res):
    st, xo, b1, _ = ic.exact(case, k)
    if res.success != (st == 0):
        return False
    if st != 0:
        return True
    M, p = case[0], ic.problem(case, k)
    if not ic.close(float(np.dot(p["c"], res.x)), b1):
        return False
    return not ic.unique(case, k) or np.array_equal(np.rint(res.x[:2 * M]), xo[:2 * M])


def test_exact_oracle_matches_highs():
    """HiGHS (mip_gap None) against the exact oracle on every instance: status, c.x within 1e-9 relative, the
    rounded (w, n) where unique. A case where HiGHS with presolve departs (the fractional-slack class, DESIGN.md
    §9) is compared with the presolve-off answer, counted, and capped at 5 %."""
    from scipy.optimize import Bounds, LinearConstraint, milp

    inst = ic.instances()
    nopre = []
    for case, k in inst:
        p = ic.problem(case, k)
        if _highs_agrees(case, k, mo.highs_solve(p, mip_gap=None)):
            continue
        nopre.append((case, k))
        cons = [LinearConstraint(p["A_ub"], -np.inf, p["b_ub"]), LinearConstraint(p["A_eq"], p["b_eq"], p["b_eq"])]
        res = milp(c=p["c"], integrality=p["integrality"], bounds=Bounds(p["lb"], p["ub"]), constraints=cons,
                   options={"time_limit": 3600.0, "presolve": False})
        assert _highs_agrees(case, k, res), (case, k)
    print(f"HiGHS = exact oracle on {len(inst) - len(nopre)} of {len(inst)}; presolve-off class: {nopre}")
    assert len(nopre) <= 0.05 * len(inst), nopre


# ------------------------------------------------------------------ plan pricing
def test_numpy_plan_evaluation_prices_optima_and_neighbours():
    """evaluate_plan_np prices every oracle optimum to the oracle's objective (and its slack / t columns), and
    two single-layer neighbours per instance (one layer moved; one n_i + 1) to HiGHS with w and n fixed."""
    rng = np.random.default_rng(pc.NEIGHBOUR_SEED)
    feas = infeas = 0
    for c in ic.CASES:
        M, model, kvf = c[0], ic.model_of(c), ic.kv_factor(c[3])
        t = fleet_table([ic.devices(c)], model)
        for k in ic.ks_of(M):
            st, xo, _, _ = ic.exact(c, k)
            if st != 0:
                continue
            w, n = [int(v) for v in np.rint(xo[:M])], [int(v) for v in np.rint(xo[M:2 * M])]
            e = pl.evaluate_plan_np(t, model, 0, k, w, n, kvf)
            assert e.feasible and e.reason == 0, (c, k, e.reason)
            assert ic.close(e.obj_value, ic.objective(c, k)), (c, k, e.obj_value, ic.objective(c, k))
            ic.check_x(e.x, c, k, "evaluate_plan_np")
            nb = ic.neighbours(rng, w, n)
            for kind, w2, n2 in nb:
                e = pl.evaluate_plan_np(t, model, 0, k, w2, n2, kvf)
                ok, obj = ic.price_fixed(c, k, w2, n2)
                assert e.feasible == ok, (c, k, kind, w2, n2, e.reason)
                if ok:
                    feas += 1
                    assert ic.close(e.obj_value, obj), (c, k, kind, e.obj_value, obj)
                else:
                    infeas += 1
                    assert e.reason != 0 and e.obj_value == np.inf and e.bottleneck == -1
    print(f"neighbours: {feas} feasible, {infeas} infeasible")
    assert feas >= 50 and infeas >= 20, (feas, infeas)


# ------------------------------------------------------------------ the reference's recorded results
@pytest.fixture(scope="module")
def golden():
    return load_json("irregular.json")


def test_irregular_golden_is_data_of_the_case_list(golden):
    fleets = golden["fleets"]
    assert (golden["kv_bits"], golden["mip_gap"]) == ("4bit", 1e-4)
    assert [ic.case_of_record(f) for f in fleets] == ic.golden_cases() and 25 <= len(fleets) <= 40
    names = {e for f in fleets for e in f["edits"]}
    assert names == {e for e in ic.EDIT_NAMES if e.split(":")[-1] not in ("31", "32", "63", "66")}
    for f in fleets:
        assert set(f) == {"M", "scale", "seed", "edits", "result", "error", "per_k"}
        assert (f["error"] is None) == (f["result"] is not None)
        if f["error"] is None:
            assert [r["k"] for r in f["per_k"]] == list(ic.ks_all(f["M"]))


@pytest.mark.parametrize("solver", ["exact", "highs"])
def test_oracle_reproduces_the_recorded_irregular_results(golden, solver):
    for f in golden["fleets"]:
        if f["error"] is None:
            assert ic.golden_mismatch(f, solver) is None, (f["M"], f["edits"], ic.golden_mismatch(f, solver))


def test_recorded_exceptions_are_raised_by_every_host_entry(golden):
    """Where the reference raised on a profile, halda_solve, fleet_table and halda_solve_batch raise the same
    type with the same message (none needs a GPU: the packer and the host coefficients raise first). The
    reference raised on none of the 32 recorded fleets, so there is no record to check today: the test holds
    the rule for a record that a regenerated golden may bring."""
    from distilp_amd.solver import halda_solve, halda_solve_batch

    for f in golden["fleets"]:
        if f["error"] is None:
            continue
        case = ic.case_of_record(f)
        devs, model = ic.devices(case), ic.model_of(case)
        name, _, msg = f["error"].partition(": ")
        for call in (lambda: halda_solve(devs, model, mip_gap=1e-4, plot=False, kv_bits="4bit"),
                     lambda: fleet_table([devs], model),
                     lambda: halda_solve_batch([devs], model, mip_gap=1e-4, kv_bits="4bit")):
            with pytest.raises(Exception) as info:
                call()
            assert (type(info.value).__name__, str(info.value)) == (name, msg), (case, info.value)
