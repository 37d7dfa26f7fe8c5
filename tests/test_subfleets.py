"""Sub-fleets of a packed table (distilp_amd/solver/subfleets.py), host side: argument errors, the chunk
planner, the NumPy-gathered item table against fleet_table of the materialised lists, halda_select_devices'
rules with an injected solve, and the exact oracle pinned to tests/golden/subfleets.json. No GPU."""

import ctypes
import types

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, fleet_table

from .conftest import load_json
from .subfleets_cases import golden_mismatch, our_devices, our_model
from .test_abi import kernel_resources


def test_new_entry_points_are_exported_and_reject_null():
    for name in ("halda_solve_subfleets", "halda_solve_subfleets_host", "halda_set_subfleets_path",
                 "halda_last_subfleets_route"):
        assert name in lh.EXPORTS
    raw = ctypes.CDLL(str(lh.LIB_PATH))
    lib = lh.load_library()
    raw.halda_set_subfleets_path.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert raw.halda_set_subfleets_path(None, 0) == -22
    raw.halda_last_subfleets_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert raw.halda_last_subfleets_route(None, None) == -22
    raw.halda_solve_subfleets_host.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_void_p]
    assert raw.halda_solve_subfleets_host(None, None, None, None, None, 1, None) == -22
    assert "NULL" in lh.last_error(lib)
    import distilp.solver
    import distilp_amd.solver

    for mod in (distilp.solver, distilp_amd.solver):
        for name in ("halda_solve_subfleets", "halda_leave_one_out", "halda_leave_one_out_batch",
                     "halda_select_devices"):
            assert getattr(mod, name) is getattr(sf, name)


def test_item_validation_errors():
    sizes = np.asarray([3, 5])
    with pytest.raises(IndexError, match="device index 3 out of range"):
        sf.pack_items(sizes, [(1, [0, 4]), (0, [0, 3])])
    with pytest.raises(IndexError, match="device index -1"):
        sf.pack_items(sizes, [(0, [-1])])
    with pytest.raises(ValueError, match="item 1: empty"):
        sf.pack_items(sizes, [(0, [0]), (1, [])])
    with pytest.raises(IndexError, match="fleet index 2 out of range"):
        sf.pack_items(sizes, [(2, [0])])
    with pytest.raises(IndexError, match="fleet index -1"):
        sf.pack_items(sizes, [(-1, [0])])
    parent, off, idx = sf.pack_items(sizes, [(1, [4, 4, 0]), (0, (2,))])
    assert (parent.dtype, off.dtype, idx.dtype) == (np.int32, np.int64, np.int32)
    assert (parent.tolist(), off.tolist(), idx.tolist()) == ([1, 0], [0, 3, 4], [4, 4, 0, 2])
    # the public entry raises them before it packs a device or touches a GPU
    devs = our_devices(7200, 2)
    with pytest.raises(IndexError):
        sf.halda_solve_subfleets([devs], our_model(), [(0, [2])])
    with pytest.raises(ValueError):
        sf.halda_solve_subfleets([devs], our_model(), [(0, [])])
    with pytest.raises(IndexError):
        sf.halda_solve_subfleets([devs], our_model(), [(1, [0])])


def test_chunk_planner_splits_at_item_boundaries():
    assert sf.plan_chunks([], 10) == []
    assert sf.plan_chunks([3, 3, 3], 100) == [(0, 3)]
    assert sf.plan_chunks([3, 3, 3], 6) == [(0, 2), (2, 3)]
    assert sf.plan_chunks([3, 3, 3], 5) == [(0, 1), (1, 2), (2, 3)]
    assert sf.plan_chunks([7, 1, 1, 9, 2], 4) == [(0, 1), (1, 3), (3, 4), (4, 5)]  # a longer item: its own chunk
    rng = np.random.default_rng(0)
    lens = rng.integers(1, 20, 200).tolist()
    chunks = sf.plan_chunks(lens, 64)
    assert chunks[0][0] == 0 and chunks[-1][1] == len(lens)
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert all(sum(lens[a:b]) <= 64 for a, b in chunks)
    assert all(sum(lens[a:b + 1]) > 64 for a, b in chunks[:-1])  # greedy: the next item would not fit
    assert sf.SUBFLEET_CHUNK_DEVICES == 1 << 21


def test_leave_one_out_items():
    parent, off, idx = sf.leave_one_out_items([3, 1, 2])
    assert parent.tolist() == [0, 0, 0, 2, 2]
    assert off.tolist() == [0, 2, 4, 6, 7, 8]
    assert idx.tolist() == [1, 2, 0, 2, 0, 1, 1, 0]
    parent, off, idx = sf.leave_one_out_items([1])
    assert len(parent) == 0 and off.tolist() == [0] and len(idx) == 0


def test_gathered_table_equals_the_packed_materialised_lists():
    """Headless lists (device 0, the only is_head one, dropped), repeats, reversed order, several parents."""
    model = our_model()
    fleets = [our_devices(7300, 3), our_devices(7800, 8), our_devices(8600, 16)]
    assert all(devs[0].is_head and not any(d.is_head for d in devs[1:]) for devs in fleets)
    items = [(1, [1, 2, 3, 4, 5, 6, 7]), (0, [2, 1, 0]), (2, list(range(15, -1, -1))), (1, [3, 3, 0, 3]), (0, [1]),
             (2, [5, 0, 5]), (1, [7]), (2, list(range(1, 16)))]
    table = fleet_table(fleets, model)
    got = sf.gather_table(table, *sf.pack_items(table.sizes(), items))
    want = fleet_table([[fleets[f][j] for j in s] for f, s in items], model)
    for f in ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    assert np.array_equal(got._heads, want._heads)
    assert got._heads.tolist()[:4] == [0, 7 + 2, 10 + 15, 26 + 2]  # headless: first listed; else the is_head one
    for a, b in zip(got._blocks, want._blocks):
        assert a.flags["C_CONTIGUOUS"] and np.array_equal(a, b)
    # a table without the packer's blocks (field arrays only) gathers the same
    plain = types.SimpleNamespace(**{f: getattr(table, f) for f in ("dev_off", "os_class", "flags") + F64_FIELDS
                                     + BYTE_FIELDS})
    again = sf.gather_table(plain, *sf.pack_items(table.sizes(), items))
    assert all(np.array_equal(getattr(again, f), getattr(want, f)) for f in F64_FIELDS + BYTE_FIELDS + ("flags",))


def test_item_table_equals_the_materialised_constants(monkeypatch):
    """item_table (the C packer's consts_items on the parent table and the index arrays) gives, bit for bit,
    fleet_constants, the classes and the kappa heads of fleet_table of the materialised lists; so does its
    fallback through gather_table."""
    from distilp_amd.solver.fleets import fleet_constants

    model = our_model()
    fleets = [our_devices(7300, 3), our_devices(7800, 8), our_devices(8600, 16), our_devices(7200, 2)]
    items = [(1, [1, 2, 3, 4, 5, 6, 7]), (0, [2, 1, 0]), (2, list(range(15, -1, -1))), (1, [3, 3, 0, 3]), (0, [1]),
             (2, [5, 0, 5]), (1, [7]), (2, list(range(1, 16))), (3, [1]), (3, [1, 0])]
    items += [(2, [j for j in range(16) if j != i]) for i in range(16)]
    table = fleet_table(fleets, model)
    arrays = sf.pack_items(table.sizes(), items)
    want = fleet_table([[fleets[f][j] for j in s] for f, s in items], model)
    consts = fleet_constants(want, model)
    g = np.repeat(table.dev_off[arrays[0].astype(np.int64)], np.diff(arrays[1])) + arrays[2]

    def check(it):
        assert np.array_equal(it.dev_off, want.dev_off) and it.n_fleets == len(items)
        assert np.array_equal(it.sizes(), want.sizes())
        assert it.os_class.dtype == np.uint8 and np.array_equal(it.os_class, want.os_class)
        assert np.array_equal(it.heads, g[want._heads])
        for a, b in zip(it.consts, consts):
            assert a.tobytes() == np.ascontiguousarray(b).tobytes()

    assert hasattr(sf._PACKER, "consts_items")
    check(sf.item_table(table, *arrays, model))
    monkeypatch.setattr(sf, "_PACKER", None)
    check(sf.item_table(table, *arrays, model))
    monkeypatch.undo()
    # the C helper checks what it indexes
    bad = arrays[2].copy()
    bad[5] = 8
    with pytest.raises(ValueError, match="consts_items"):
        sf.item_table(table, arrays[0], arrays[1], bad, model)
    # a list whose own head has s_disk 0 raises the packer's ZeroDivisionError (kappa divides by it)
    t2 = fleet_table([fleets[1]], model)
    t2.s_disk[4] = 0.0  # a row of the packed block
    for lst in ([4, 1], [1, 2]):  # device 4 as the list's head; not listed at all
        args = sf.pack_items(t2.sizes(), [(0, lst)])
        if lst[0] == 4:
            with pytest.raises(ZeroDivisionError):
                sf.item_table(t2, *args, model)
        else:
            sf.item_table(t2, *args, model)


def test_a_head_without_b1_raises_as_the_materialised_fleet_does():
    """With "b_1" in f_out but not in f_q, a CPU FLOPs row without "b_1" is an error on kappa's head only: the
    parent packs, a list that makes the device its head raises the packer's ValueError, other lists do not."""
    model = our_model().model_copy(update={"f_q": {k: v for k, v in our_model().f_q.items() if k != "b_1"}})
    devs = our_devices(7800, 8)
    row = {k: v for k, v in devs[3].scpu[model.Q].items() if k != "b_1"}
    devs[3] = devs[3].model_copy(update={"scpu": dict(devs[3].scpu, **{model.Q: row})})
    devs[5] = devs[5].model_copy(update={"scpu": {k: v for k, v in devs[5].scpu.items() if k != model.Q}})
    table = fleet_table([devs], model)  # device 3 is not the parent's head: it packs
    for lst, raises in (([3, 1, 2], True), ([1, 3, 2], False), ([0, 3], False), ([5, 3], False), ([3], True)):
        arrays = sf.pack_items(table.sizes(), [(0, [1, 2]), (0, lst)])
        heads = sf.item_table(table, *arrays, model).heads
        if raises:
            with pytest.raises(ValueError, match="Batch size 1") as mine:
                sf.check_item_heads([devs], table, arrays[0], heads, model)
            with pytest.raises(ValueError) as theirs:
                fleet_table([[devs[j] for j in lst]], model)
            assert str(mine.value) == str(theirs.value)
            with pytest.raises(ValueError, match="Batch size 1"):  # the public entry, before any GPU call
                sf.halda_solve_subfleets([devs], model, [(0, [1, 2]), (0, lst)])
        else:
            sf.check_item_heads([devs], table, arrays[0], heads, model)
            fleet_table([[devs[j] for j in lst]], model)
    sf.check_item_heads([devs], table, arrays[0], heads, our_model())  # with f_q: nothing left to the head


def _fake_solver(objs):
    """solve_lists over a table {frozenset of kept indices: obj_value or None}; records the calls."""
    calls = []

    def solve(lists):
        calls.append([list(s) for s in lists])
        out = []
        for s in lists:
            v = objs.get(frozenset(s), 100.0 + len(s))
            out.append(None if v is None else types.SimpleNamespace(obj_value=v, kept=list(s)))
        return out

    return solve, calls


def test_select_devices_stopping_and_tie_rules():
    devs = ["a", "b", "c", "d"]
    full = frozenset(range(4))
    # round 1: dropping 1 or 2 ties at 5.0 -> the lowest index (1); round 2: nothing is strictly below 5.0
    solve, calls = _fake_solver({full: 9.0, full - {1}: 5.0, full - {2}: 5.0, full - {0}: 7.0,
                                 frozenset({0, 2}): 5.0, frozenset({0, 3}): 5.0, frozenset({2, 3}): 6.0})
    kept, r = sf.halda_select_devices(devs, None, _solve_lists=solve)
    assert kept == [0, 2, 3] and r.obj_value == 5.0 and r.kept == [0, 2, 3]
    assert calls == [[[0, 1, 2, 3]], [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], [[2, 3], [0, 3], [0, 2]]]
    # no removal improves: the full fleet, after one round
    solve, calls = _fake_solver({full: 1.0})
    kept, r = sf.halda_select_devices(devs, None, _solve_lists=solve)
    assert kept == [0, 1, 2, 3] and r.obj_value == 1.0 and len(calls) == 2
    # an equal objective is no improvement
    solve, _ = _fake_solver({full: 5.0, full - {3}: 5.0})
    assert sf.halda_select_devices(devs, None, _solve_lists=solve)[0] == [0, 1, 2, 3]
    # every removal improves: down to one device, and it stops there (no empty list is ever solved)
    solve, calls = _fake_solver({frozenset(s): float(len(s)) for s in
                                 [(0, 1, 2, 3), (1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2), (2, 3), (1, 3), (1, 2),
                                  (3,), (2,)]})
    kept, r = sf.halda_select_devices(devs, None, _solve_lists=solve)
    assert kept == [3] and r.obj_value == 1.0  # every round ties: device 0, then 1, then 2 goes
    assert all(len(s) >= 1 for c in calls for s in c)
    # an infeasible fleet: any feasible removal improves; nothing feasible at all raises
    solve, _ = _fake_solver({full: None, full - {0}: None, full - {2}: 50.0})
    assert sf.halda_select_devices(devs, None, _solve_lists=solve)[0] == [0, 1, 3]
    solve, _ = _fake_solver({frozenset(s): None for s in [(0, 1), (0,), (1,)]})
    with pytest.raises(RuntimeError, match="No feasible MILP"):
        sf.halda_select_devices(devs[:2], None, _solve_lists=solve)
    solve, calls = _fake_solver({})
    assert sf.halda_select_devices(devs[:1], None, _solve_lists=solve)[0] == [0] and len(calls) == 1


def test_exact_oracle_matches_the_recorded_reference_on_every_leave_one_out_list():
    G = load_json("subfleets.json")
    assert (G["kv_bits"], G["mip_gap"]) == ("8bit", 1e-4)
    assert sorted({f["M"] for f in G["fleets"]}) == [2, 3, 8, 16]
    n = 0
    for fl in G["fleets"]:
        assert [rec["drop"] for rec in fl["lists"]] == list(range(fl["M"]))  # every list, the headless one too
        for rec in fl["lists"]:
            assert rec["error"] is None
            why = golden_mismatch(our_devices(fl["seed"], fl["M"], rec["drop"]), our_model(), rec, G["kv_bits"])
            assert why is None, (fl["M"], fl["seed"], rec["drop"], why)
            n += 1
    assert n == sum(f["M"] for f in G["fleets"])


def test_fused_kernel_uses_no_scratch(tmp_path):
    """halda_sweep_subfleets_kernel keeps every value in registers at halda_sweep_kernel's occupancy (four
    waves per SIMD: at most 128 VGPRs)."""
    res = kernel_resources(tmp_path)
    r = res["halda_sweep_subfleets_kernel"]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 128, r
    assert "halda_expand_subfleets_kernel" in res
