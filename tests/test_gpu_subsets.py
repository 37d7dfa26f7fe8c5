"""Exact device selection on the GPU (libhalda halda_solve_subsets): per (fleet, d) the frontier's raw obj and
best_k equal the strict earliest-index arg-min over the raw obj_value / best_k that halda_solve_subfleets (the
C entry) writes for every enumerated list, on the fused route (halda_sweep_subsets_kernel) and the expansion
route (halda_subsets_index_kernel), and the Python entries built on them agree with the brute force over the
exact oracle."""

import contextlib
import ctypes
import io
import itertools
import math

import numpy as np
import pytest

from distilp_amd.solver import (halda_leave_one_out, halda_select_devices_exact, halda_solve_subfleets,
                                halda_subset_frontier, halda_subset_frontier_batch)
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import subsets as ss
from distilp_amd.solver.fleets import fleet_table, model_struct

from . import pressure_cases as pc
from . import subsets_cases as sc
from .conftest import REPO
from .subfleets_cases import our_devices, our_model
from .test_gpu_subfleets import KS80, _torch, _upload, fleet, solve_items_device

pytestmark = pytest.mark.gpu

INFEASIBLE = lh.STATUS_INFEASIBLE


def solve_subsets_device(table, model, D, keep_masks=None, ks=KS80, path=0, stream=None):
    """halda_solve_subsets on a device copy of `table`: (status, obj, dropped_mask, best_k) [nf, D + 1], route."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    lib = ctx.lib
    arrs, fs = _upload(table)
    n = table.n_fleets * (D + 1)
    o = {"status": torch.full((n,), -7, dtype=torch.int32, device=dev),
         "obj": torch.full((n,), -7.0, dtype=torch.float64, device=dev),
         "mask": torch.full((n,), -7, dtype=torch.int64, device=dev),
         "best_k": torch.full((n,), -7, dtype=torch.int32, device=dev)}
    fr = ss.HaldaSubsetFrontierC(*[o[f].data_ptr() for f in ("status", "obj", "mask", "best_k")])
    km = None if keep_masks is None else np.asarray(keep_masks, np.uint64)
    sub = ss.HaldaSubsetsC(D, None if km is None else km.ctypes.data)
    karr = np.asarray(ks, np.int32)
    m = model_struct(model, 0.5)
    torch.cuda.synchronize(dev)
    ss.set_subsets_path(ctx, path)
    try:
        with ctx._lock:
            rc = lib.halda_solve_subsets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
                                         karr.ctypes.data, len(ks), ctypes.byref(fr),
                                         ctypes.c_void_p(stream.cuda_stream) if stream is not None else None)
    finally:
        ss.set_subsets_path(ctx, 0)
    assert rc == 0, lh.last_error(lib)
    torch.cuda.synchronize(dev)
    shape = (table.n_fleets, D + 1)
    return (o["status"].cpu().numpy().reshape(shape), o["obj"].cpu().numpy().reshape(shape),
            o["mask"].cpu().numpy().view(np.uint64).reshape(shape), o["best_k"].cpu().numpy().reshape(shape),
            ss.last_subsets_route(ctx))


def mask_of(devs):
    return sum(1 << i for i in devs)


def check_frontier(fleets, model, D, keeps=None, paths=(0, 1), sample=None, route0=None, ks=KS80):
    """The frontier of each path against halda_solve_subfleets of the enumerated lists (every candidate, or
    with `sample` a seeded sample of that many per (fleet, d) plus the frontier's winners)."""
    table = fleet_table(fleets, model)
    keeps = keeps or [()] * len(fleets)
    masks = [mask_of(k) for k in keeps] if any(keeps) else None
    rng = np.random.default_rng(20261020)
    out = None
    for p in paths:
        st, obj, dm, bk, route = solve_subsets_device(table, model, D, masks, ks, p)
        assert route == ("expand" if p == 1 else route0 or route), (p, route)
        assert not (st == -7).any() and not (bk == -7).any()
        items, groups = [], {}
        for f, devs in enumerate(fleets):
            M = len(devs)
            for d in range(D + 1):
                if d > sc.limit_of(M, keeps[f], None):
                    assert (st[f, d], obj[f, d], dm[f, d], bk[f, d]) == (INFEASIBLE, math.inf, 0, 0), (f, d)
                    continue
                cands = sc.candidates(M, keeps[f], d)
                pick = list(range(len(cands)))
                if sample is not None and len(cands) > sample:
                    pick = sorted(set(rng.choice(len(cands), sample, replace=False).tolist()) |
                                  {j for j, (g, _) in enumerate(cands) if mask_of(g) == int(dm[f, d])})
                groups[(f, d)] = (len(items), pick, cands)
                items += [(f, list(cands[j][1])) for j in pick]
        want = solve_items_device(table, items, model, ks)
        for (f, d), (a, pick, cands) in groups.items():
            o = want["obj_value"][a:a + len(pick)]
            j = int(np.flatnonzero(o == o.min())[0])  # strict <: the earliest minimum
            what = (p, f, d, pick[j])
            assert obj[f, d].tobytes() == o[j].tobytes(), what
            assert bk[f, d] == want["best_k"][a + j], what
            if o[j] < math.inf:
                assert st[f, d] == lh.STATUS_OPTIMAL and int(dm[f, d]) == mask_of(cands[pick[j]][0]), what
            else:
                assert st[f, d] == INFEASIBLE and dm[f, d] == 0, what
        if out is not None:
            for a, b in zip(out, (st, obj, dm, bk)):
                assert a.tobytes() == b.tobytes(), "the routes differ"
        out = (st, obj, dm, bk)
    return out


@pytest.mark.parametrize("seed,M,D", sc.IDENTITY_CASES)
def test_frontier_equals_the_arg_min_over_every_candidate_on_both_routes(llama_online_model, seed, M, D):
    devs = fleet(M, seed)
    D = M - 1 if D is None else D
    st, obj, dm, bk = check_frontier([devs], llama_online_model, D)
    assert dm[0, 0] == 0 and st.shape == (1, D + 1)
    assert ss.subsets_count(M, D) == sum(len(sc.candidates(M, (), d)) for d in range(D + 1))


def test_fused_route_three_fleets_of_64_with_keep(llama_online_model):
    """2,081 candidates per fleet (2,081 - 64 - 63 - ... with two devices kept on fleet 1), one wave each."""
    fleets = [fleet(64, 4300 + s) for s in range(3)]
    keeps = [(), (0, 5), ()]
    st, obj, dm, bk = check_frontier(fleets, llama_online_model, 2, keeps, paths=(0,), sample=200, route0="fused")
    assert ss.subsets_count(64, 2) == 2081
    assert not (int(dm[1, 1]) | int(dm[1, 2])) & mask_of(keeps[1])
    # point 1 is the best leave-one-out list (the Python entries: host-formed objectives)
    pts = halda_subset_frontier(fleets[0], llama_online_model, 2)
    loo = halda_leave_one_out(fleets[0], llama_online_model)
    objs = [math.inf if r is None else r.obj_value for r in loo]
    i = int(np.argmin(objs))
    assert pts[1].obj_value == objs[i] and pts[1].dropped == [i]
    assert lh.get_context(0) and ss.last_subsets_route(lh.get_context(0)) == "fused"
    # the expansion route on a sample of the same call: the same frontier bits
    st1, obj1, dm1, bk1, route = solve_subsets_device(fleet_table(fleets, llama_online_model), llama_online_model, 2,
                                                      [mask_of(k) for k in keeps], path=1)
    assert route == "expand"
    for a, b in ((st, st1), (obj, obj1), (dm, dm1), (bk, bk1)):
        assert a.tobytes() == b.tobytes()


def test_mixed_batch_of_five_sizes(llama_online_model):
    fleets = [fleet(M, 4400 + M) for M in (1, 2, 7, 16, 64)]
    st, obj, dm, bk = check_frontier(fleets, llama_online_model, 1, paths=(0,))
    assert (st[0, 1], obj[0, 1], dm[0, 1]) == (INFEASIBLE, math.inf, 0)  # one device: the single point d = 0
    out = halda_subset_frontier_batch(fleets, llama_online_model, 1)
    assert [len(p) for p in out] == [1, 2, 2, 2, 2]
    assert ss.last_subsets_route(lh.get_context(0)) in ("expand", "mixed")


@pytest.mark.parametrize("case", sc.ENTRY_CASES)
def test_python_entries_against_the_brute_force(case):
    seed, M, D, keep = case
    devs, model = our_devices(seed, M), our_model()
    pts = halda_subset_frontier(devs, model, D, keep)
    bf = sc.brute_force(*case)
    assert len(pts) == len(bf)
    assert pts[0].dropped == [] and pts[0].kept == list(range(M))
    for d, (p, (best, gone, runner)) in enumerate(zip(pts, bf)):
        if gone is None:
            assert p.result is None and p.obj_value == math.inf
            continue
        assert len(p.dropped) == d and not set(p.dropped) & set(keep)
        assert abs(p.obj_value - best) <= sc.REL_OBJ * max(1.0, abs(best)), (d, p.obj_value, best)
        if not sc.near_tie(best, runner):
            assert tuple(p.dropped) == tuple(gone), (d, p.dropped, gone)
        same = halda_solve_subfleets([devs], model, [(0, p.kept)])[0]
        assert (p.result.k, p.result.w, p.result.n, p.result.sets) == (same.k, same.w, same.n, same.sets)
        assert np.float64(p.result.obj_value).tobytes() == np.float64(same.obj_value).tobytes()
    kept, r = halda_select_devices_exact(devs, model, D, keep)
    best = min(b for b, _, _ in bf)
    assert abs(r.obj_value - best) <= sc.REL_OBJ * max(1.0, abs(best))
    winners = [p for p in pts if p.result is not None and p.obj_value == r.obj_value]
    assert kept == winners[0].kept  # among equal objectives the fewest drops


# ------------------------------------------------------------------ memory pressure and moved heads
def case_id(case):
    key, D, keep = case
    name = f"p{key[1]}s{key[3]}" if key[0] == "p" else f"i{key[1][0]}{key[1][4][0]}"
    return f"{name}-D{D}-keep{''.join(map(str, keep))}"


@pytest.mark.parametrize("case", sc.PRESSURE_CASES, ids=case_id)
def test_frontier_under_pressure_and_with_moved_heads(case):
    """Both routes on a pressured or head-edited fleet: the raw frontier equals the arg-min over every candidate's
    halda_solve_subfleets value bit for bit (check_frontier), the routes agree bit for bit, the 64-device fleets
    take the fused route; and the raw objective equals the brute force over the exact oracle within 1e-9, the
    dropped set too wherever the runner-up is no near tie."""
    key, D, keep = case
    devs, model, kv, ks = sc.fleet_of(key)
    M = len(devs)
    D = sc.limit_of(M, keep, D)
    ks = list(KS80 if ks is None else ks)
    st, obj, dm, bk = check_frontier([devs], model, D, [keep], ks=ks, route0="fused" if M == 64 else None)
    bf = sc.brute_force_of(*case)
    assert len(bf) == D + 1
    for d, (best, gone, runner) in enumerate(bf):
        if gone is None:
            assert st[0, d] == INFEASIBLE and obj[0, d] == math.inf
            continue
        assert st[0, d] == lh.STATUS_OPTIMAL, (case, d)
        assert abs(obj[0, d] - best) <= sc.REL_OBJ * max(1.0, abs(best)), (case, d, obj[0, d], best)
        assert not int(dm[0, d]) & mask_of(keep)
        if not sc.near_tie(best, runner):
            assert int(dm[0, d]) == mask_of(gone), (case, d, int(dm[0, d]), gone)


@pytest.mark.parametrize("edit", ["two_heads", "head_at:last", "no_head"])
def test_a_candidate_that_drops_the_head_gets_the_documented_head(edit):
    """The head of a kept list is its first is_head device, else its first device: the lists that drop device 0,
    the head, and both, through halda_solve_subfleets (what a candidate's value is) and through the frontier with
    those devices the only droppable ones, each against the exact oracle on that kept list."""
    key = next(k for k, _, keep in sc.PRESSURE_CASES if k[0] == "i" and k[1][4] == (edit,) and k[1][0] == 16)
    devs, model, kv, ks = sc.fleet_of(key)
    M = len(devs)
    head = next((i for i, d in enumerate(devs) if d.is_head), 0)
    last = max(i for i, d in enumerate(devs) if d.is_head) if any(d.is_head for d in devs) else M - 1
    drops = sorted({(0,), (head,), (last,), tuple(sorted({0, last}))})
    lists = [[i for i in range(M) if i not in g] for g in drops]
    got = halda_solve_subfleets([devs], model, [(0, kept) for kept in lists], k_candidates=list(ks), kv_bits=kv)
    for g, kept, r in zip(drops, lists, got):
        want = sc.oracle_of(key, tuple(kept))
        assert r is not None and want is not None, (edit, g)
        assert abs(r.obj_value - want["obj_value"]) <= sc.REL_OBJ * max(1.0, abs(want["obj_value"])), (edit, g, r, want)
        assert r.sets == want["sets"], (edit, g)
    keep = [i for i in range(M) if i not in (0, last)]
    pts = halda_subset_frontier(devs, model, None, keep, k_candidates=list(ks), kv_bits=kv)
    bf = sc.brute_force_of(key, None, tuple(keep))
    assert len(pts) == len(bf) >= 2
    for p, (best, gone, runner) in zip(pts, bf):
        assert abs(p.obj_value - best) <= sc.REL_OBJ * max(1.0, abs(best)), (edit, p.dropped, p.obj_value, best)
        if not sc.near_tie(best, runner):
            assert tuple(p.dropped) == tuple(gone), (edit, p.dropped, gone)


def test_an_infeasible_group_has_no_plan():
    seed, M, scale = sc.STARVED
    devs, model = pc.devices(seed, M, scale), pc.our_model()
    keep = (sc.starved_keep(),)
    st, obj, dm, bk = check_frontier([devs], model, M - 1, [keep])
    assert st[0].tolist() == [lh.STATUS_OPTIMAL] * (M - 1) + [INFEASIBLE]
    assert (obj[0, M - 1], dm[0, M - 1]) == (math.inf, 0)
    pts = halda_subset_frontier(devs, model, keep=keep)
    assert len(pts) == M and all(p.result is not None for p in pts[:-1])
    assert pts[-1].result is None and pts[-1].obj_value == math.inf and pts[-1].dropped == []
    assert halda_select_devices_exact(devs, model, keep=keep)[1].obj_value == min(p.obj_value for p in pts)


def test_a_second_call_on_another_stream_gives_the_same_bits(llama_online_model):
    torch, dev = _torch()
    fleets = [fleet(64, 4300), fleet(64, 4301)]
    table = fleet_table(fleets, llama_online_model)
    a = solve_subsets_device(table, llama_online_model, 1)
    b = solve_subsets_device(table, llama_online_model, 1, stream=torch.cuda.Stream(dev))
    c = solve_subsets_device(table, llama_online_model, 1, path=1, stream=torch.cuda.Stream(dev))
    assert (a[4], b[4], c[4]) == ("fused", "fused", "expand")
    for x, y, z in zip(a[:4], b[:4], c[:4]):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_cli_prints_the_frontier_and_the_selection():
    from distilp_amd.cli import solver as cli

    assert REPO.exists()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(["--profile", "hermes_70b", "--no-plot", "--quiet", "--select-devices"])
    assert rc in (0, None)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith(("drop ", "selected:"))]
    assert lines[0].startswith("drop 0: dropped=[], k=") and " obj=" in lines[0]
    assert lines[-1].startswith("selected: kept=[")
    assert len(lines) >= 2
