"""Exact device selection (distilp_amd/solver/subsets.py), host side: the combo lists and their order, the
slot -> device mapping under `keep`, the selection logic through `_solve_lists` backed by the exact oracle
against a brute force over itertools.combinations, the tie order, every argument error, and the new
kernels' code-object metadata. No GPU."""

import ctypes
import itertools
import math
import types

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver import subsets as ss

from . import subsets_cases as sc
from .subfleets_cases import our_devices, our_model
from .test_abi import kernel_resources


def test_new_entry_points_are_exported_and_reject_bad_arguments():
    names = ("halda_solve_subsets", "halda_solve_subsets_host", "halda_subsets_count", "halda_last_subsets_route",
             "halda_set_subsets_path")
    assert all(n in lh.EXPORTS for n in names)
    raw = ctypes.CDLL(str(lh.LIB_PATH))
    lib = lh.load_library()
    assert lib.halda_version() == 3  # additive: the ABI version stays
    raw.halda_set_subsets_path.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert raw.halda_set_subsets_path(None, 0) == -22
    raw.halda_last_subsets_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert raw.halda_last_subsets_route(None, None) == -22
    raw.halda_solve_subsets_host.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_void_p]
    assert raw.halda_solve_subsets_host(None, None, None, None, None, 1, None) == -22
    assert "NULL" in lh.last_error(lib)
    raw.halda_solve_subsets.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    assert raw.halda_solve_subsets(None, None, None, None, None, 1, None, None) == -22
    import distilp.solver
    import distilp_amd.solver

    for mod in (distilp.solver, distilp_amd.solver):
        for name in ("halda_subset_frontier", "halda_subset_frontier_batch", "halda_select_devices_exact",
                     "SubsetPoint"):
            assert getattr(mod, name) is getattr(ss, name)


@pytest.mark.parametrize("q", [1, 3, 6, 16])
def test_combo_lists_are_itertools_combinations_in_the_stated_order(q):
    lib = lh.load_library()
    total = 0
    for d in range(0, min(q, 3) + 1):
        combos = ss.combo_list(q, d)
        want = list(itertools.combinations(range(q), d))
        assert [tuple(r for r in range(q) if (c >> r) & 1) for c in combos] == want
        assert want == sorted(want)  # ascending index lists, lexicographic
        total += len(combos)
        assert lib.halda_subsets_count(q, d) == ss.subsets_count(q, d) == total
    assert ss.subsets_count(q, 99) == 2 ** q == lib.halda_subsets_count(q, 99)


def test_subsets_count_limits():
    lib = lh.load_library()
    assert lib.halda_subsets_count(64, 2) == 2081 and lib.halda_subsets_count(16, 16) == 65536
    assert lib.halda_subsets_count(20, 20) == ss.SUBSETS_MAX == 1 << 20
    assert lib.halda_subsets_count(64, 64) == 2 ** 63 - 1  # saturated
    assert [lib.halda_subsets_count(*a) for a in ((-1, 0), (65, 0), (3, -1))] == [-1, -1, -1]
    assert lib.halda_subsets_count(0, 0) == 1


def test_slot_to_device_mapping_under_keep():
    assert ss.droppable(6, None) == [0, 1, 2, 3, 4, 5]
    slots = ss.droppable(6, [4, 1])
    assert slots == [0, 2, 3, 5]
    assert ss.combo_devices(slots, 0b0101) == [0, 3] and ss.combo_devices(slots, 0b1000) == [5]
    got = list(ss.candidate_lists(6, slots, 2))
    assert got[0] == ([0, 2], [1, 3, 4, 5]) and got[-1] == ([3, 5], [0, 1, 2, 4]) and len(got) == 6
    assert [g for g, _ in got] == [list(c) for c in itertools.combinations(slots, 2)]
    for bad in ([6], [-1], [True], [1.0]):
        with pytest.raises(IndexError, match="out of range"):
            ss.droppable(6, bad)


@pytest.mark.parametrize("case", sc.HOST_CASES)
def test_frontier_equals_the_brute_force_minimum(case):
    seed, M, D, keep = case
    devs, model, solve = our_devices(seed, M), our_model(), sc.oracle_solver(seed, M)
    pts = ss.halda_subset_frontier(devs, model, D, keep, _solve_lists=solve)
    bf = sc.brute_force(*case)
    assert len(pts) == len(bf) == sc.limit_of(M, keep, D) + 1
    for d, (p, (best, gone, _)) in enumerate(zip(pts, bf)):
        assert p.obj_value == best and tuple(p.dropped) == gone and len(p.dropped) == d
        assert sorted(p.dropped + p.kept) == list(range(M)) and p.result.kept == p.kept
        assert not set(p.dropped) & set(keep)
    full = solve([list(range(M))])[0]
    assert pts[0].kept == list(range(M)) and pts[0].obj_value == full.obj_value  # point 0 is the full fleet
    kept, r = ss.halda_select_devices_exact(devs, model, D, keep, _solve_lists=solve)
    assert r.obj_value == min(b for b, _, _ in bf) and r.kept == kept
    first = [d for d, (b, _, _) in enumerate(bf) if b == r.obj_value][0]
    assert len(kept) == M - first  # among equal objectives the fewest drops


def test_exact_selection_is_never_worse_than_the_greedy_walk():
    better = 0
    cases = [c for c in sc.HOST_CASES if c[2] is None and not c[3]]
    for seed, M, D, keep in cases:
        devs, model, solve = our_devices(seed, M), our_model(), sc.oracle_solver(seed, M)
        _, exact = ss.halda_select_devices_exact(devs, model, _solve_lists=solve)
        _, greedy = sf.halda_select_devices(devs, model, _solve_lists=solve)
        assert exact.obj_value <= greedy.obj_value, (seed, M)
        better += exact.obj_value < greedy.obj_value
    print(f"exact selection strictly better than greedy on {better} of {len(cases)} fleets")
    assert len(cases) == 4


def test_ties_go_to_the_earliest_candidate_and_the_fewest_drops():
    """One device repeated: every candidate of one d ties, so the first combination wins; a later d wins only
    when strictly lower."""
    devs = [our_devices(9103, 3)[1]] * 4
    by_len = {4: 5.0, 3: 4.0, 2: 4.0, 1: 7.0}

    def solve(lists):
        return [types.SimpleNamespace(obj_value=by_len[len(s)], kept=list(s)) for s in lists]

    pts = ss.halda_subset_frontier(devs, None, _solve_lists=solve)
    assert [p.dropped for p in pts] == [[], [0], [0, 1], [0, 1, 2]]
    kept, r = ss.halda_select_devices_exact(devs, None, _solve_lists=solve)
    assert kept == [1, 2, 3] and r.obj_value == 4.0  # d = 2 ties with d = 1: the fewer drops
    pts = ss.halda_subset_frontier(devs, None, 2, keep=[0], _solve_lists=solve)
    assert [p.dropped for p in pts] == [[], [1], [1, 2]]

    def none(lists):
        return [None for _ in lists]

    pts = ss.halda_subset_frontier(devs, None, _solve_lists=none)
    assert all(p.result is None and p.obj_value == math.inf and p.dropped == [] for p in pts) and len(pts) == 4
    with pytest.raises(RuntimeError, match="No feasible MILP found for any k this round."):
        ss.halda_select_devices_exact(devs, None, _solve_lists=none)


def test_argument_errors_are_raised_without_a_gpu():
    model = our_model()
    devs = our_devices(9105, 5)
    with pytest.raises(ValueError, match="at most 64 devices"):
        ss.halda_subset_frontier(devs * 13, model)
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="max_drop"):
            ss.halda_subset_frontier(devs, model, bad)
    with pytest.raises(ValueError, match="beyond"):
        ss.halda_subset_frontier(devs, model, 5)  # M - 1 = 4
    with pytest.raises(ValueError, match="beyond"):
        ss.halda_subset_frontier(devs, model, 3, keep=[0, 1, 2])  # q = 2
    with pytest.raises(IndexError, match="out of range"):
        ss.halda_subset_frontier(devs, model, 1, keep=[5])
    with pytest.raises(IndexError):
        ss.halda_subset_frontier([], model)
    with pytest.raises(ValueError, match=r"2097152 candidate.*limit of 1048576"):
        ss.halda_select_devices_exact((devs * 5)[:22], model, 21, keep=[0])
    with pytest.raises(ValueError, match="keep entries"):
        ss.halda_subset_frontier_batch([devs, devs], model, keep=[[0]])
    assert ss.halda_subset_frontier_batch([], model) == []
    ss.check_count(20, 20)  # exactly the limit


def test_a_candidate_head_without_b1_raises_before_any_gpu_work():
    """The head rule of subfleets.py on every head a candidate can have: device 3 becomes kappa's head once
    devices 0 .. 2 are dropped, which max_drop = 3 admits and max_drop = 2 does not."""
    model = our_model().model_copy(update={"f_q": {k: v for k, v in our_model().f_q.items() if k != "b_1"}})
    devs = our_devices(7800, 8)
    row = {k: v for k, v in devs[3].scpu[model.Q].items() if k != "b_1"}
    devs[3] = devs[3].model_copy(update={"scpu": dict(devs[3].scpu, **{model.Q: row})})
    with pytest.raises(ValueError, match="Batch size 1"):
        ss.halda_subset_frontier(devs, model, 3)
    flags = np.asarray([1, 0, 0, 0, 0, 0, 0, 0], np.uint8) * sf.DEV_HEAD
    assert ss.possible_heads(flags, list(range(8)), 2) == [0, 1, 2]
    assert ss.possible_heads(flags, list(range(8)), 3) == [0, 1, 2, 3]
    assert ss.possible_heads(flags, list(range(1, 8)), 7) == [0]  # the head is kept: always the head
    assert ss.possible_heads(np.zeros(4, np.uint8), [0, 1, 2, 3], 3) == [0, 1, 2, 3]


def test_near_ties_stay_inside_the_cap():
    """The GPU test may skip the kept-set comparison at near-tie points only: by the oracle alone they are at
    most a quarter of the points of its seeds."""
    pts = [(b, r) for case in sc.ENTRY_CASES for b, g, r in sc.brute_force(*case) if g is not None]
    near = sum(sc.near_tie(b, r) for b, r in pts)
    print(f"near-tie points: {near} of {len(pts)}")
    assert near <= sc.NEAR_TIE_CAP * len(pts)


def test_near_ties_of_the_pressured_and_moved_head_cases_stay_inside_the_cap():
    """The same cap over sc.PRESSURE_CASES (pressured fleets, fleets with two heads, the head last or none), by
    the oracle alone; and the cases are what they are meant to be: dropping devices pushes the rest of a
    pressured fleet into slacks, and some candidate drops the head."""
    from oracle import milp_oracle as mo

    pts = [(b, r) for case in sc.PRESSURE_CASES for b, g, r in sc.brute_force_of(*case) if g is not None]
    near = sum(sc.near_tie(b, r) for b, r in pts)
    print(f"near-tie points: {near} of {len(pts)}")
    assert len(pts) >= 40 and near <= sc.NEAR_TIE_CAP * len(pts)
    key = sc.PRESSURE_CASES[0][0]
    devs, model, kv, _ = sc.fleet_of(key)
    used = 0
    for kept in itertools.combinations(range(5), 2):
        r = sc.oracle_of(key, kept)
        prob = mo.lower_dense([devs[i] for i in kept], model, r["k"], mo._kv_factor(kv))
        st, x, *_ = mo.exact_solve(prob)
        used += st == 0 and bool((x[4:12] > 0.5).any())  # a slack or a t column is in use at the best k
    print(f"two-device sub-fleets whose optimum uses a slack: {used} of 10")
    assert used >= 1  # the full fleet uses none at its best k: dropping devices is what brings the slacks in
    heads = {k[1][4][0] for k, _, keep in sc.PRESSURE_CASES if k[0] == "i" and keep}
    assert heads == {"two_heads", "head_at:last", "no_head"}


def test_new_kernels_use_no_scratch(tmp_path):
    """halda_sweep_subsets_kernel keeps the register sweep's occupancy (four waves per SIMD: at most 128
    VGPRs, no scratch, no spills)."""
    res = kernel_resources(tmp_path)
    r = res["halda_sweep_subsets_kernel"]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 128, r
    for k in ("halda_subsets_index_kernel", "halda_subsets_pick_kernel"):
        assert res[k]["private_segment_fixed_size"] == 0, res[k]
