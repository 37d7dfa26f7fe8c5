"""Scale-in / scale-out on the GPU (halda_solve_change_subsets): the raw grid against the strict earliest arg-min
over halda_solve_change on EVERY enumerated list, chunked runs against the one-chunk run, the Python entries against
tests/golden/scale.json and change.json, the identities with the failover, change and join entries, the gate, and
a call on another stream between two other users of the context's scratch."""

import ctypes
import math

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import change as ch
from distilp_amd.solver import scale as sc
from distilp_amd.solver import subsets as ss
from distilp_amd.solver.fleets import _host_struct, fleet_table, model_struct
from distilp_amd.solver.subfleets import pack_items

from . import bounds_cases as bc
from . import change_cases as cc
from . import scale_cases as sx
from .deep_cases import model_at
from .test_abi import kernel_resources

pytestmark = pytest.mark.gpu

KVB = "4bit"  # kv factor 0.5, bounds_cases.KV
FIELDS = ("status", "obj", "dropped_mask", "loaded", "released", "w", "n")


def masks_of(fleets, keeps):
    return None if keeps is None else np.asarray([sc._mask(k or ()) for k in keeps], np.uint64)


def raw_scale(model, fleets, k, w0s, dmin, dmax, P, keeps=None):
    table = fleet_table(fleets, model)
    w0 = np.concatenate([np.asarray(w, np.int32) for w in w0s])
    return sc.solve_change_subsets_table(table, model, k, w0, dmin, dmax, P, bc.KV, masks_of(fleets, keeps))


def spec_scale(model, fleets, k, w0s, dmin, dmax, P, keeps=None):
    """The grid by full enumeration: per d ONE halda_solve_change call over every candidate of every fleet, then
    the strict earliest arg-min per (fleet, p) on its raw obj, the winner's planes scattered to parent order.
    Also {(fleet, d): candidates} and {(fleet, d, p): the winner's candidate index}."""
    nf, D1, P1 = len(fleets), dmax - dmin + 1, P + 1
    out = sc.ScaleSolve(status=np.full((nf, D1, P1), lh.STATUS_INFEASIBLE, np.int32), obj=np.full((nf, D1, P1), np.inf),
                        dropped_mask=np.zeros((nf, D1, P1), np.uint64), loaded=np.zeros((nf, D1, P1), np.int32),
                        released=np.zeros((nf, D1, P1), np.int32), w=np.zeros((nf, D1, P1, 64), np.int32),
                        n=np.zeros((nf, D1, P1, 64), np.int32), k=k, min_drop=dmin, max_drop=dmax, max_p=P)
    table = fleet_table(fleets, model)
    count, win = {}, {}
    for d in range(dmin, dmax + 1):
        items, group = [], []
        for f, devs in enumerate(fleets):
            slots = ss.droppable(len(devs), None if keeps is None else keeps[f])
            cands = list(ss.candidate_lists(len(devs), slots, d)) if d <= min(len(slots), len(devs) - 1) else []
            count[(f, d)] = len(cands)
            for c, (gone, kept) in enumerate(cands):
                items.append((f, kept))
                group.append((f, c, gone, kept))
        if not items:
            continue
        packed = pack_items(table.sizes(), items)
        w0 = np.concatenate([np.asarray([w0s[f][i] for i in kept], np.int32) for f, kept in items])
        res = ch.solve_change_table(table, model, k, packed, w0, P, bc.KV)
        for p in range(P1):
            for i, (f, c, gone, kept) in enumerate(group):
                if res.status[i, p] == lh.STATUS_OPTIMAL and res.obj[i, p] < out.obj[f, d - dmin, p]:  # strict
                    a = int(packed[1][i])
                    out.status[f, d - dmin, p] = lh.STATUS_OPTIMAL
                    out.obj[f, d - dmin, p] = res.obj[i, p]
                    out.dropped_mask[f, d - dmin, p] = sc._mask(gone)
                    out.loaded[f, d - dmin, p] = res.loaded[i, p]
                    out.released[f, d - dmin, p] = res.released[i, p]
                    out.w[f, d - dmin, p] = 0
                    out.n[f, d - dmin, p] = 0
                    out.w[f, d - dmin, p, kept] = res.w[p, a:a + len(kept)]
                    out.n[f, d - dmin, p, kept] = res.n[p, a:a + len(kept)]
                    win[(f, d, p)] = c
    return out, count, win


def same(a, b, tag):
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (tag, f)


def stale(model, M, k, s):
    if M <= 5:
        return cc.stale_parent(model, M, k, s)
    return list(bc.devices(M, s)), list(bc.incumbent_w(model, M, k, s))


# (name, [(M, k, seed)], k, d range, P, keep per fleet)
SHAPES = [(f"M{M}_k{k}_P{P}", [(M, k, 0)], k, (0, 2), P, None) for M in (4, 5, 8) for k in (1, 2) for P in (0, 3)]
SHAPES += [("M16_two_kept", [(16, 2, 0)], 2, (0, 2), 2, [[0, 7]]), ("M64_lane63", [(64, 1, 0)], 1, (0, 1), 2, None),
           ("mixed_3_5_8", [(3, 2, 0), (5, 2, 0), (8, 2, 0)], 2, (0, 3), 2, None)]
_CALLS = {}


def shape_call(model, name):
    """(fleets, k, w0s, dmin, dmax, P, keeps, got, want, count, win) of a shape, solved once."""
    if name not in _CALLS:
        _, parents, k, (dmin, dmax), P, keeps = next(s for s in SHAPES if s[0] == name)
        fleets, w0s = zip(*(stale(model, M, k, s) for M, _, s in parents))
        fleets, w0s = list(fleets), list(w0s)
        got = raw_scale(model, fleets, k, w0s, dmin, dmax, P, keeps)
        want, count, win = spec_scale(model, fleets, k, w0s, dmin, dmax, P, keeps)
        _CALLS[name] = (fleets, k, w0s, dmin, dmax, P, keeps, got, want, count, win)
    return _CALLS[name]


# ------------------------------------------------------------------ 1. identity with the full enumeration
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_grid_equals_the_enumerated_arg_min(llama_online_model, name):
    fleets, k, w0s, dmin, dmax, P, keeps, got, want, count, win = shape_call(llama_online_model, name)
    same(got, want, name)
    assert (got.status[:, 0] == lh.STATUS_OPTIMAL).any(), name
    if name == "mixed_3_5_8":
        assert count[(0, 3)] == 0 and (got.status[0, 3] == lh.STATUS_INFEASIBLE).all() and np.isinf(got.obj[0, 3]).all()
        assert not got.w[0, 3].any() and (got.status[1:, 3, -1] == lh.STATUS_OPTIMAL).all()
    if name == "M64_lane63":
        assert count[(0, 1)] == 64 and (got.w[0, 0, -1] >= 1).all()  # lane 63 holds a device; lists of 63
    if name == "M16_two_kept":
        assert not (got.dropped_mask & np.uint64(sc._mask([0, 7]))).any() and count[(0, 2)] == 91


def test_scale_out_parent_with_zero_w0_and_min_drop(llama_online_model):
    """devs + pool, the pool's w0 zero, every device of devs kept, min_drop = q - 2 > 0."""
    model = llama_online_model
    devs, w, pool = sx.out_case(model)
    fleets, w0s, keeps = [devs + pool], [list(w) + [0] * len(pool)], [list(range(len(devs)))]
    got = raw_scale(model, fleets, 1, w0s, 1, 3, sx.P, keeps)
    want, count, _ = spec_scale(model, fleets, 1, w0s, 1, 3, sx.P, keeps)
    same(got, want, "out")
    assert [count[(0, d)] for d in (1, 2, 3)] == [3, 3, 1]
    assert (got.status[0, :2, 0] == lh.STATUS_INFEASIBLE).all()  # a joiner needs a layer: point 0 has no plan
    assert got.status[0, 0, 1] == lh.STATUS_INFEASIBLE  # two joiners need two layers
    assert (got.status[0, 2] == lh.STATUS_OPTIMAL).all() and (got.status[0, 1, 1:] == lh.STATUS_OPTIMAL).all()
    assert (got.status[0, 0, 2:] == lh.STATUS_OPTIMAL).all()


# ------------------------------------------------------------------ 2. chunks
@pytest.mark.parametrize("name,per", [("M5_k2_P3", 1), ("M8_k2_P3", 2), ("M8_k1_P3", 1), ("mixed_3_5_8", 1),
                                      ("M16_two_kept", 4)])
def test_chunked_run_is_byte_identical(llama_online_model, name, per):
    """The cap holds `per` candidates of the longest list, so every (fleet, d) group of 3 * per or more candidates
    spans at least three launches; some winner sits past its group's first launch."""
    model = llama_online_model
    fleets, k, w0s, dmin, dmax, P, keeps, got, _, count, win = shape_call(model, name)
    ctx = lh.get_context(0)
    cap = sc.launch_bytes(max(len(d) for d in fleets), P, per)
    lib = ctx.lib
    assert lib.halda_change_subsets_launch_bytes(max(len(d) for d in fleets), P, per) == cap
    sc.set_change_subsets_chunk(ctx, cap)
    try:
        again = raw_scale(model, fleets, k, w0s, dmin, dmax, P, keeps)
    finally:
        sc.set_change_subsets_chunk(ctx, 0)
    same(again, got, name)
    # a launch holds at most n0 = (cap - fixed) // (bytes of one candidate of the group) of a group's candidates: a
    # group of 3 n0 or more spans at least three launches, and a winner of index >= n0 sits past the group's first
    n0 = {(f, d): max(1, (cap - sc.FIXED_BYTES) // (sc.launch_bytes(len(fleets[f]) - d, P, 1) - sc.FIXED_BYTES))
          for (f, d), n in count.items() if n}
    wide = [g for g, n in count.items() if n and n >= 3 * n0[g]]
    assert wide and any(c >= n0[(f, d)] for (f, d, p), c in win.items() if (f, d) in wide), (name, win)


# ------------------------------------------------------------------ 3. the Python entries against the oracle
def check_row(row, W, w0, tag):
    last = math.inf
    for p, pt in enumerate(row):
        assert pt.point.obj_value <= last, (tag, p)
        last = pt.point.obj_value
        if pt.point.plan is not None:
            D = W - sum(w0[i] for i in pt.kept)
            assert pt.point.loaded == D + pt.point.released and pt.point.released <= p, (tag, p)
            assert sorted(pt.dropped + pt.kept) == list(range(len(w0))), (tag, p)


@pytest.mark.parametrize("M,k,s", sx.PARENTS + sx.EXTRA)
def test_scale_in_equals_the_oracle(llama_online_model, M, k, s):
    """Rows d = 1 and d = 2 against the recorded minima (feasibility exact, 1e-9 relative -- DESIGN 4.9's
    tolerance), loaded = deficit + released, rows non-increasing in p; each point equals the failover entry's bit
    for bit; row 0 is the change frontier of the whole fleet; halda_scale_in returns row d's last point."""
    model, gold = llama_online_model, sx.golden()
    devs, w = cc.stale_parent(model, M, k, s)
    inc = (k, w, [0] * M)
    fr = sc.halda_scale_in_frontier(devs, model, inc, 2, sx.P, kv_bits=KVB)
    assert len(fr) == 3 and all(len(r) == sx.P + 1 for r in fr)
    single = cc.golden()["S"]
    for p in sx.PS:
        cell = gold["cells"][f"{M},{k},{s}"][str(p)]
        pt = fr[2][p]
        assert (pt.point.plan is None) == (cell["obj"] is None), (M, k, s, p)
        if cell["obj"] is not None:
            assert bc.rel(pt.point.obj_value, cell["obj"]) <= 1e-9, (M, k, s, p, pt.point.obj_value, cell)
            rec = gold["pairs"][sx.pair_key(M, k, s, pt.dropped)]
            assert bc.rel(rec["obj"][str(p)], cell["obj"]) <= 1e-9 and len(pt.dropped) == 2, (M, k, s, p, pt.dropped)
        if (M, k, s) in sx.PARENTS:  # d = 1: the minimum over `lost` of change.json's point p
            ones = [single[cc.key(M, k, s, i)]["obj"][str(p)] for i in range(M)]
            _, least = sx.best(ones)
            assert (fr[1][p].point.plan is None) == (least is None)
            assert least is None or bc.rel(fr[1][p].point.obj_value, least) <= 1e-9, (M, k, s, p)
    for d, row in enumerate(fr):
        check_row(row, int(model.L) // k, w, (M, k, s, d))
        lost = {tuple(pt.dropped) for pt in row if pt.point.plan is not None}
        by = {g: ch.halda_failover_frontiers(devs, model, inc, sx.P, [g], KVB)[0] for g in lost if g}
        for p, pt in enumerate(row):
            if pt.point.plan is None:
                assert pt.dropped == [] and pt.kept == [] and pt.point == ch.ChangePoint(p, None, math.inf, 0, 0, math.inf)
            elif d:
                assert len(pt.dropped) == d and pt.point == by[tuple(pt.dropped)][p], (M, k, s, d, p)
    assert [pt.point for pt in fr[0]] == ch.halda_change_frontier(devs, model, k, w, sx.P, KVB)
    gone, plan = sc.halda_scale_in(devs, model, inc, 2, sx.P, kv_bits=KVB)
    assert gone == fr[2][-1].dropped and plan == fr[2][-1].point.plan


def test_the_exact_pick_beats_the_greedy_pair(llama_online_model):
    """Per (M, k) group some d = 2 cell whose recorded winner is strictly better than the greedy repeat of the best
    single loss: there the entry returns the winner, not the greedy pair."""
    model, gold = llama_online_model, sx.golden()
    seen = set()
    for M, k, s in sx.PARENTS + sx.EXTRA:
        cells = gold["cells"][f"{M},{k},{s}"]
        ps = [p for p in sx.PS if cells[str(p)]["greedy"] is not None and cells[str(p)]["pair"] != cells[str(p)]["greedy"]
              and cells[str(p)]["obj"] < gold["pairs"][sx.pair_key(M, k, s, cells[str(p)]["greedy"])]["obj"][str(p)]
              * (1 - 1e-9 if cells[str(p)]["obj"] > 0 else 1 + 1e-9) - 1e-9]
        if not ps:
            continue
        devs, w = cc.stale_parent(model, M, k, s)
        row = sc.halda_scale_in_frontier(devs, model, (k, w, [0] * M), 2, sx.P, min_drop=2, kv_bits=KVB)[0]
        for p in ps:
            assert row[p].dropped == cells[str(p)]["pair"] != cells[str(p)]["greedy"], (M, k, s, p)
        seen.add((M, k))
    assert seen == {(M, k) for M, k, _ in sx.PARENTS} - sx.NO_GAP


def test_batch_of_two_ks_equals_the_single_calls(llama_online_model):
    model = llama_online_model
    cases = [(4, 1, 0), (5, 2, 0), (5, 1, 1)]
    fleets, incs = [], []
    for M, k, s in cases:
        devs, w = cc.stale_parent(model, M, k, s)
        fleets.append(devs)
        incs.append((k, w, [0] * M))
    got = sc.halda_scale_in_frontier_batch(fleets, model, incs, 2, 2, keep=[[0], None, None], kv_bits=KVB)
    for f, (devs, inc) in enumerate(zip(fleets, incs)):
        assert got[f] == sc.halda_scale_in_frontier(devs, model, inc, 2, 2, keep=[0] if f == 0 else None, kv_bits=KVB)
    assert all(0 in pt.kept for row in got[0] for pt in row if pt.point.plan is not None)


def test_scale_out_equals_the_oracle_and_the_join_entry(llama_online_model):
    model, gold = llama_online_model, sx.golden()["out"]
    devs, w, pool = sx.out_case(model)
    k, inc = sx.OUT[1], (sx.OUT[1], w, [0] * len(devs))
    fr = sc.halda_scale_out_frontier(devs, pool, model, inc, sx.OUT_ADD, sx.P, KVB)
    assert len(fr) == sx.OUT_ADD + 1
    for a, row in enumerate(fr):
        keys = [key for key in gold if (0 if key == "none" else len(key.split("+"))) == a]
        for p in sx.PS:
            _, least = sx.best([gold[key]["obj"][str(p)] for key in keys])
            assert (row[p].point.plan is None) == (least is None), (a, p)
            if least is not None:
                assert bc.rel(row[p].point.obj_value, least) <= 1e-9 and len(row[p].added) == a, (a, p)
                assert bc.rel(gold[sx.out_key(row[p].added)]["obj"][str(p)], least) <= 1e-9, (a, p)
                assert row[p].kept == list(range(len(devs))) + [len(devs) + j for j in row[p].added]
        check_row(row, int(model.L) // k, list(w) + [0] * len(pool), ("out", a))
    assert [pt.point for pt in fr[0]] == ch.halda_change_frontier(devs, model, k, w, sx.P, KVB)
    joins = ch.halda_join_frontiers(devs, pool, model, inc, sx.P, KVB)
    for p in range(sx.P + 1):
        # the dropped-list order: among equal objectives the LAST pool device is the earliest candidate
        order = sorted(range(len(pool)), reverse=True)
        at, _ = sx.best([joins[j][p].obj_value if joins[j][p].plan is not None else None for j in order])
        if at is None:
            assert fr[1][p].point.plan is None
        else:
            assert fr[1][p].added == [order[at]] and fr[1][p].point == joins[order[at]][p], p


# ------------------------------------------------------------------ 4. the gate
def c_call(model, devs, k, w0, dmin, dmax, P, keep=0):
    """halda_solve_change_subsets_host on one fleet: (rc, status array prefilled with -9)."""
    ctx = lh.get_context(0)
    lib = ctx.lib
    table = fleet_table([devs], model)
    fs, hold = _host_struct(table)
    m = model_struct(model, bc.KV)
    pts = (dmax - dmin + 1) * (P + 1)
    st = np.full(pts, -9, np.int32)
    obj, mask = np.zeros(pts), np.zeros(pts, np.uint64)
    ld, rl = np.zeros(pts, np.int32), np.zeros(pts, np.int32)
    w, n = np.zeros(pts * 64, np.int32), np.zeros(pts * 64, np.int32)
    a, km = np.asarray(w0, np.int32), np.asarray([keep], np.uint64)
    sub = sc.HaldaChangeSubsetsC(a.ctypes.data, None, None, dmin, dmax, P, km.ctypes.data)
    fr = sc.HaldaChangeSubsetFrontierC(*(x.ctypes.data for x in (st, obj, mask, ld, rl, w, n)))
    with ctx._lock:
        rc = lib.halda_solve_change_subsets_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), k, ctypes.byref(sub),
                                                 ctypes.byref(fr))
    del hold
    return rc, st


def test_gate_inside_and_outside(llama_online_model):
    """One case just inside and one just outside each of 2 P + Dmax_d <= 254, the LDS budget and the 2^20
    candidates; the outside ones are refused (HALDA_E_ARG, ValueError) and nothing is written."""
    ctx = lh.get_context(0)
    lib = ctx.lib
    # (a) 2 P + Dmax_d <= 254 on a 250-layer model: three devices, d = 1 drops the one that holds 243
    deep = model_at(llama_online_model, 250)
    devs = list(bc.devices(3, 0))
    w0 = [243, 4, 3]
    assert sc.max_deficit(w0, [0, 1, 2], 1, 250) == 243
    for P, ok in ((5, True), (6, False)):  # 2 P + 243 = 253, 255
        assert (2 * P + 243 <= ch.MAX_ENTRY) == ok and ch.change_lds_bytes(2, P, 243, 1) <= ch.LDS_BUDGET
        rc, st = c_call(deep, devs, 1, w0, 0, 1, P)
        assert (rc == 0) == ok and (ok or (rc == -22 and "254" in lh.last_error(lib) and (st == -9).all())), (P, rc)
        if ok:
            assert (st != -9).all()
        else:
            with pytest.raises(ValueError, match="254"):
                sc.halda_scale_in_frontier(devs, deep, (1, w0, [0, 0, 0]), 1, P, kv_bits=KVB)
            # d = 0 alone is inside: a small d is not gated by a large d's deficit
            assert c_call(deep, devs, 1, w0, 0, 0, P)[0] == 0
    # (b) the LDS budget: 8 devices at k = 1, one of them holding 73 layers: the largest P of d = 1's gate, and one more
    model = llama_online_model
    devs8, w8 = list(bc.devices(8, 0)), [int(model.L) - 7] + [1] * 7
    D1 = sc.max_deficit(w8, list(range(8)), 1, int(model.L))
    Pin = min(cc.gate_p(ch, 8, 0, 1), cc.gate_p(ch, 7, D1, 1))
    assert D1 == 73 and 0 <= Pin < ch.MAX_P and 2 * (Pin + 1) + D1 <= ch.MAX_ENTRY  # the next P fails on LDS alone
    rc, st = c_call(model, devs8, 1, w8, 0, 1, Pin)
    assert rc == 0 and (st != -9).all()
    rc, st = c_call(model, devs8, 1, w8, 0, 1, Pin + 1)
    assert rc == -22 and "LDS" in lh.last_error(lib) and (st == -9).all()
    with pytest.raises(ValueError, match="LDS"):
        sc.halda_scale_in_frontier(devs8, model, (1, w8, [0] * 8), 1, Pin + 1, kv_bits=KVB)
    # (c) 2^20 candidates: 21 droppable devices of 22 have 2^20 subsets of d <= 10 (C(21, 0..10) = 2^20), 22 have more
    assert sc.scale_count(21, 22, 0, 10) == 1 << 20 and sc.scale_count(22, 22, 0, 10) > 1 << 20
    devs22 = list(bc.devices(22, 0))
    w22 = [int(model.L) - 21] + [1] * 21
    with pytest.raises(ValueError, match="exceed"):
        sc.halda_scale_in_frontier(devs22, model, (1, w22, [0] * 22), 10, 0, kv_bits=KVB)
    rc, st = c_call(model, devs22, 1, w22, 0, 10, 0)
    assert rc == -22 and "candidates" in lh.last_error(lib) and (st == -9).all()
    sc.check_scale_gate([22], [list(range(1, 22))], [w22], int(model.L), 1, 0, 10, 0)  # inside, by the arithmetic
    rc, st = c_call(model, devs22, 1, w22, 10, 10, 0)  # inside on the device: C(22, 10) = 646,646 candidates
    assert rc == 0 and (st != -9).all()


def test_other_refusals_before_any_launch(llama_online_model):
    model = llama_online_model
    devs, w = cc.stale_parent(model, 4, 1, 0)
    lib = lh.get_context(0).lib
    for args in ((w, 2, 1, 0), (w, 0, 64, 0), (w, 0, 1, 64), (w, 0, 1, -1), (w, 4, 4, 0), ([81, 1, 1, 1], 0, 1, 0),
                 ([-1, 1, 1, 1], 0, 1, 0)):
        rc, st = c_call(model, devs, 1, *args)
        assert rc == -22 and (st == -9).all(), args
    rc, st = c_call(model, devs, 1, w, 0, 1, 0, keep=1 << 4)
    assert rc == -22 and "keep_mask" in lh.last_error(lib)
    rc, st = c_call(model, devs, 1, w, 3, 3, 0, keep=1)  # q = 3, M - 1 = 3: admitted
    assert rc == 0
    w0 = np.asarray(w, np.int32)
    assert lib.halda_change_subsets_max_deficit(w0.ctypes.data, 4, 1, 2, 80) == sc.max_deficit(w, [1, 2, 3], 2, 80)
    assert lib.halda_change_subsets_max_deficit(w0.ctypes.data, 4, 1, 4, 80) == -1


def test_new_kernels_code_objects(tmp_path):
    """No scratch memory and no spilled registers in the two new kernels."""
    res = kernel_resources(tmp_path)
    for name in ("halda_change_subsets_index_kernel", "halda_change_subsets_pick_kernel"):
        r = res[name]
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r


# ------------------------------------------------------------------ 5. streams
def test_call_on_another_stream_between_two_scratch_users(llama_online_model):
    """halda_solve_change_subsets on a non-default stream, enqueued between two halda_solve_subsets calls on the
    context's stream (both use the context's selection scratch): the same bytes as the host entry's."""
    import torch

    from distilp_amd.solver.fleets import DeviceFleetTable

    model = llama_online_model
    fleets, k, w0s, dmin, dmax, P, keeps, got, _, _, _ = shape_call(model, "M8_k2_P3")
    dev = torch.device("cuda", 0)
    ctx = lh.get_context(0)
    lib = ctx.lib
    table = fleet_table(fleets, model)
    dt = DeviceFleetTable(table, model, [k], bc.KV, dev)
    nf, D1, P1 = len(fleets), dmax - dmin + 1, P + 1
    w0 = torch.from_numpy(np.concatenate([np.asarray(w, np.int32) for w in w0s])).to(dev)
    outs = {f: torch.zeros((nf, D1, P1) + ((64,) if f in ("w", "n") else ()),
                           dtype={"obj": torch.float64, "dropped_mask": torch.int64}.get(f, torch.int32), device=dev)
            for f in FIELDS}
    sub = sc.HaldaChangeSubsetsC(w0.data_ptr(), None, None, dmin, dmax, P, None)
    fr = sc.HaldaChangeSubsetFrontierC(*(outs[f].data_ptr() for f in FIELDS))
    m = model_struct(model, bc.KV)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    before = ss.solve_subsets_table(table, model, [k], bc.KV, 2, None)
    with ctx._lock:
        rc = lib.halda_solve_change_subsets(ctx.ctx, ctypes.byref(m), ctypes.byref(dt.fs), k,
                                            ctypes.byref(sub), ctypes.byref(fr), s.cuda_stream)
    assert rc == 0, lh.last_error(lib)
    after = ss.solve_subsets_table(table, model, [k], bc.KV, 2, None)
    torch.cuda.synchronize(dev)
    for f in FIELDS:
        assert outs[f].cpu().numpy().tobytes() == getattr(got, f).tobytes(), f
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
