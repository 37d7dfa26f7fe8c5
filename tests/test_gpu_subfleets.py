"""Sub-fleets of a resident table on the GPU (libhalda halda_solve_subfleets): every output of an item
equals, bit for bit, what halda_solve_fleets writes for the fleet of its listed devices materialised --
through the fused route (halda_sweep_subfleets_kernel), the expansion route
(halda_expand_subfleets_kernel) and the Python entries built on them -- and the reference's recorded
leave-one-out results (tests/golden/subfleets.json)."""

import contextlib
import ctypes
import io

import numpy as np
import pytest

from distilp_amd.common import DeviceProfile
from distilp_amd.solver import (halda_leave_one_out, halda_leave_one_out_batch, halda_select_devices,
                                halda_solve_batch, halda_solve_subfleets)
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaFleetResultC, _fleets_struct, _host_struct,
                                       fleet_table, model_struct, open_x_offsets)
from distilp_amd.synth import synth_fleet

from .conftest import REPO, load_json
from .helpers import synth_devices
from .subfleets_cases import exact_sweep, our_devices, result_mismatch

pytestmark = pytest.mark.gpu

KS80 = [1, 2, 4, 5, 8, 10, 16, 20, 40]  # the default k list of the 80-layer model
OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c")
TABLE_FIELDS = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS


def fleet(M, seed):
    return synth_devices(M, seed, synth_fleet(seed, M))


def leave_one_out(parent, M):
    return [(parent, [j for j in range(M) if j != i]) for i in range(M)]


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _upload(table):
    torch, dev = _torch()
    arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in TABLE_FIELDS}
    return arrs, _fleets_struct(table, lambda f: arrs[f].data_ptr())


def _results(n, tot, nk, xlen, x_off=None):
    """Device result arrays (x / c zeroed: the dense layout's tail past 7 M + 1 is never written)."""
    torch, dev = _torch()
    o = {"best_k": torch.full((n,), -7, dtype=torch.int32, device=dev),
         "obj_value": torch.full((n,), -7.0, dtype=torch.float64, device=dev),
         "w": torch.full((tot,), -7, dtype=torch.int32, device=dev),
         "n": torch.full((tot,), -7, dtype=torch.int32, device=dev),
         "obj_by_k": torch.full((n * nk,), -7.0, dtype=torch.float64, device=dev),
         "status": torch.full((n * nk,), -7, dtype=torch.int32, device=dev),
         "x": torch.zeros(xlen, dtype=torch.float64, device=dev),
         "c": torch.zeros(xlen, dtype=torch.float64, device=dev)}
    xo = None if x_off is None else torch.from_numpy(x_off).to(dev)
    r = HaldaFleetResultC(*[o[f].data_ptr() for f in OUTS], xo.data_ptr() if xo is not None else None)
    return o, r, xo


def _xlen(sizes, nk, x_off):
    if x_off is None:
        return len(sizes) * nk * (7 * int(sizes.max()) + 1)
    return int(np.max(x_off + np.repeat(7 * sizes + 1, nk), initial=0))


def solve_fleets_device(table, model, ks, x_off=None):
    """halda_solve_fleets on a device copy of `table`: every output, as NumPy arrays."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    lib = ctx.lib
    arrs, fs = _upload(table)
    sizes, nk = table.sizes(), len(ks)
    o, r, xo = _results(table.n_fleets, table.n_devices, nk, _xlen(sizes, nk, x_off), x_off)
    karr = np.asarray(ks, np.int32)
    m = model_struct(model, 0.5)
    with ctx._lock:
        rc = lib.halda_solve_fleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, nk, ctypes.byref(r),
                                    None)
    assert rc == 0, lh.last_error(lib)
    torch.cuda.synchronize(dev)
    return {f: o[f].cpu().numpy() for f in OUTS}


def solve_items_device(table, items, model, ks, path=0, x_off=None, stream=None):
    """halda_solve_subfleets on device copies of `table` and the item arrays: every output."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    lib = ctx.lib
    arrs, fs = _upload(table)
    parent, sub_off, sub_idx = sf.pack_items(table.sizes(), items)
    d = [torch.from_numpy(a).to(dev) for a in (parent, sub_off, sub_idx)]
    lens, nk = np.diff(sub_off), len(ks)
    it = sf.HaldaSubfleetsC(len(parent), int(lens.min()), int(lens.max()), *[t.data_ptr() for t in d])
    o, r, xo = _results(len(parent), int(sub_off[-1]), nk, _xlen(lens, nk, x_off), x_off)
    karr = np.asarray(ks, np.int32)
    m = model_struct(model, 0.5)
    torch.cuda.synchronize(dev)
    sf.set_subfleets_path(ctx, path)
    try:
        with ctx._lock:
            rc = lib.halda_solve_subfleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                           karr.ctypes.data, nk, ctypes.byref(r),
                                           ctypes.c_void_p(stream.cuda_stream) if stream is not None else None)
    finally:
        sf.set_subfleets_path(ctx, 0)
    assert rc == 0, lh.last_error(lib)
    torch.cuda.synchronize(dev)
    return dict({f: o[f].cpu().numpy() for f in OUTS}, route=sf.last_subfleets_route(ctx))


def assert_same_bits(got, want, what):
    for f in OUTS:
        a, b = got[f], want[f]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, f, np.flatnonzero(a != b)[:8])


def check_items(fleets, items, model, ks=KS80, paths=(0,), compact=False, route0="expand"):
    """The items' outputs on each path against halda_solve_fleets on the materialised lists; path 0 must
    have taken `route0` (the fused kernel is compared only where it really ran), path 1 the expansion."""
    table = fleet_table(fleets, model)
    mat = fleet_table([[fleets[f][j] for j in s] for f, s in items], model)
    x_off = open_x_offsets(mat, model, ks) if compact else None
    want = solve_fleets_device(mat, model, ks, x_off)
    assert not (want["best_k"] == -7).any() and not (want["status"] == -7).any() and not (want["w"] == -7).any()
    for p in paths:
        got = solve_items_device(table, items, model, ks, p, x_off)
        assert got["route"] == (route0 if p == 0 else "expand"), (p, got["route"])
        assert_same_bits(got, want, f"path {p}")
    return want


@pytest.mark.parametrize("M", [2, 3, 17, 33, 64])
def test_leave_one_out_equals_the_materialised_fleets(llama_online_model, M):
    """M = 64: the fused shape (63-device lists, k = 1 alone open); M = 17: k > 1 opens on 16-device lists;
    dropping device 0 leaves a headless list, dropping 31, 32 and 63 moves the lane boundaries."""
    devs = fleet(M, 4100 + M)
    assert devs[0].is_head and not any(d.is_head for d in devs[1:])
    # only the 63-device lists plan as the register sweep alone: 32-device lists open k = 2 (tables)
    want = check_items([devs], leave_one_out(0, M), llama_online_model, paths=(0, 1),
                       route0="fused" if M == 64 else "expand")
    assert (want["best_k"] > 0).all()
    if M == 17:  # 16-device lists: k = 2, 4 and 5 leave every device a layer, and some of them are solved
        assert (want["status"].reshape(M, -1)[:, 1:4] == lh.STATUS_OPTIMAL).any()


def test_mixed_lengths_orders_repeats_and_parents(llama_online_model):
    fleets = [fleet(12, 4201), fleet(5, 4202), fleet(30, 4203)]
    items = []
    for n in range(1, 31):  # lengths 1 .. M of each parent, the parents interleaved
        for p, devs in enumerate(fleets):
            if n <= len(devs):
                items.append((p, [(3 * j + n) % len(devs) for j in range(n)] if n % 3 == 0 else list(range(n))))
    items += [(2, list(range(29, -1, -1))), (0, [4, 4, 4, 1, 4]), (1, [3, 2, 1]), (2, [7] * 20)]
    check_items(fleets, items, llama_online_model, paths=(0,))
    check_items(fleets, items[::3], llama_online_model, compact=True)


def test_ragged_parents_of_1_to_64_devices(llama_online_model):
    fleets = [fleet(M, 4300 + M) for M in range(1, 65)]
    items = [(M - 1, [j for j in range(M) if j != (M * M // 3) % M or M == 1]) for M in range(1, 65)]
    items += [(M - 1, list(range(M))) for M in (1, 16, 17, 63, 64)]
    check_items(fleets, items, llama_online_model)


def test_lists_of_a_100_device_parent(llama_online_model):
    devs = fleet(100, 4400)
    lists = [(0, [j for j in range(100) if j != 37]), (0, list(range(90, 100))), (0, list(range(99, 0, -1))),
             (0, [0, 99, 50, 51, 52, 53, 54, 55, 56, 57])]
    check_items([devs], lists, llama_online_model, ks=[1, 2, 4, 5, 8])
    # the whole 100 devices under the default k list: 80 layers cannot give each a layer at any k
    want = check_items([devs], [(0, list(range(100)))], llama_online_model)
    assert want["best_k"].tolist() == [0] and (want["status"] == lh.STATUS_INFEASIBLE).all()
    assert np.isinf(want["obj_value"]).all() and not want["w"].any() and not want["n"].any()
    assert halda_solve_subfleets([devs], llama_online_model, [(0, list(range(100)))]) == [None]


@pytest.mark.parametrize("count", [1, 5, 257])
def test_item_counts_on_both_routes(llama_online_model, count):
    """The fused shape (63 of 64 devices) with a partial last workgroup of four waves, against path 1."""
    fleets = [fleet(64, 4500), fleet(64, 4501)]
    items = [(i % 2, [j for j in range(64) if j != (i * 7) % 64]) for i in range(count)]
    check_items(fleets, items, llama_online_model, paths=(0, 1), compact=count == 5, route0="fused")


def test_host_variant_equals_a_call_on_another_stream(llama_online_model):
    torch, dev = _torch()
    model = llama_online_model
    fleets = [fleet(64, 4600), fleet(9, 4601)]
    ctx = lh.get_context(0)
    lib = ctx.lib
    for items in (leave_one_out(0, 64), leave_one_out(1, 9) + [(0, [5, 4, 3])]):
        table = fleet_table(fleets, model)
        got = solve_items_device(table, items, model, KS80, stream=torch.cuda.Stream(dev))
        parent, sub_off, sub_idx = sf.pack_items(table.sizes(), items)
        n, tot, nk, lens = len(parent), int(sub_off[-1]), len(KS80), np.diff(sub_off)
        xlen = _xlen(lens, nk, None)
        h = {"best_k": np.empty(n, np.int32), "obj_value": np.empty(n), "w": np.empty(tot, np.int32),
             "n": np.empty(tot, np.int32), "obj_by_k": np.empty(n * nk), "status": np.empty(n * nk, np.int32),
             "x": np.zeros(xlen), "c": np.zeros(xlen)}
        r = HaldaFleetResultC(*[h[f].ctypes.data for f in OUTS], None)
        fs, keep = _host_struct(table)
        it = sf.HaldaSubfleetsC(n, 0, 0, parent.ctypes.data, sub_off.ctypes.data, sub_idx.ctypes.data)
        karr = np.asarray(KS80, np.int32)
        m = model_struct(model, 0.5)
        with ctx._lock:
            rc = lib.halda_solve_subfleets_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                karr.ctypes.data, nk, ctypes.byref(r))
        assert rc == 0, lh.last_error(lib)
        assert sf.last_subfleets_route(ctx) == got["route"] == ("fused" if lens.min() == lens.max() == 63 else "expand")
        # the dense layout's tail past an item's 7 M + 1 columns is never written: not compared
        cols = np.arange(7 * int(lens.max()) + 1)[None, :] < np.repeat(7 * lens + 1, nk)[:, None]
        for f in ("x", "c"):
            h[f], got[f] = (np.where(cols, a.reshape(n * nk, -1), 0.0) for a in (h[f], got[f]))
        assert_same_bits(h, got, "host variant")


def test_host_variant_rejects_bad_items(llama_online_model):
    model = llama_online_model
    table = fleet_table([fleet(4, 4700), fleet(2, 4701)], model)
    ctx = lh.get_context(0)
    lib = ctx.lib
    fs, keep = _host_struct(table)
    karr = np.asarray(KS80, np.int32)
    m = model_struct(model, 0.5)
    out = [np.zeros(64, np.int32), np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.int32)]
    r = HaldaFleetResultC(*[a.ctypes.data for a in out], None, None, None, None, None)
    for parent, off, idx, msg in [([0, 2], [0, 1, 2], [0, 0], "parent 2"), ([0, -1], [0, 1, 2], [0, 0], "parent -1"),
                                  ([0, 1], [0, 1, 2], [0, 2], "lists device 2"), ([0], [0, 1], [-1], "lists device -1"),
                                  ([0, 1], [0, 1, 1], [0], "empty list"), ([0], [1, 2], [0, 0], "sub_off[0]")]:
        p, o, i = np.asarray(parent, np.int32), np.asarray(off, np.int64), np.asarray(idx, np.int32)
        it = sf.HaldaSubfleetsC(len(p), 0, 0, p.ctypes.data, o.ctypes.data, i.ctypes.data)
        with ctx._lock:
            rc = lib.halda_solve_subfleets_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                karr.ctypes.data, len(KS80), ctypes.byref(r))
        assert rc == -22 and msg in lh.last_error(lib), (msg, rc, lh.last_error(lib))
    # a summary that is given must be tight (the dense x / c layout strides by max_devices)
    p, o, i = np.asarray([0, 1], np.int32), np.asarray([0, 2, 3], np.int64), np.asarray([0, 1, 0], np.int32)
    for lo, hi, ok in [(1, 2, True), (0, 0, True), (1, 3, False), (2, 2, False), (0, 2, False)]:
        it = sf.HaldaSubfleetsC(2, lo, hi, p.ctypes.data, o.ctypes.data, i.ctypes.data)
        with ctx._lock:
            rc = lib.halda_solve_subfleets_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                karr.ctypes.data, len(KS80), ctypes.byref(r))
        assert (rc == 0) if ok else (rc == -22 and "shortest and longest" in lh.last_error(lib)), (lo, hi, rc)
    with pytest.raises(RuntimeError, match="must be 0"):
        sf.set_subfleets_path(ctx, 2)


# ---------------------------------------------------------------- Python level
def _materialised(fleets, items, model, **kw):
    return [halda_solve_batch([[fleets[f][j] for j in s]], model, **kw)[0] for f, s in items]


def test_python_entries_equal_halda_solve_batch(llama_online_model, monkeypatch):
    model = llama_online_model
    fleets = [fleet(6, 4801), fleet(1, 4802), fleet(17, 4803), fleet(2, 4804)]
    items = [(0, [5, 4, 3, 2, 1, 0]), (2, list(range(1, 17))), (1, [0]), (0, [2, 2]), (3, [1]), (2, [16, 0, 8]),
             (0, [1, 2, 3, 4, 5]), (2, list(range(17)))]
    want = _materialised(fleets, items, model)
    assert halda_solve_subfleets(fleets, model, items) == want  # pydantic ==: k, w, n, sets and obj_value's bits
    assert all(r is not None for r in want)
    kw = dict(k_candidates=[1, 2, 3, 7, 40], kv_bits="4bit")
    assert halda_solve_subfleets(fleets, model, items, **kw) == _materialised(fleets, items, model, **kw)
    loo = [[halda_solve_batch([devs[:i] + devs[i + 1:]], model)[0] for i in range(len(devs))] if len(devs) > 1
           else [None] for devs in fleets]
    assert halda_leave_one_out_batch(fleets, model) == loo
    assert halda_leave_one_out(fleets[0], model) == loo[0]
    assert halda_leave_one_out(fleets[1], model) == [None]
    # the same through three chunks (40 listed devices: 5 + 16 + 1 + 2 + 1 + 3 | 5 + 17 ... split at items)
    calls = []
    real = sf.solve_items
    monkeypatch.setattr(sf, "solve_items", lambda *a, **k: calls.append(len(a[1])) or real(*a, **k))
    monkeypatch.setattr(sf, "SUBFLEET_CHUNK_DEVICES", 22)
    assert halda_solve_subfleets(fleets, model, items) == want
    assert calls == [2, 5, 1] and sum(calls) == len(items)


def test_leave_one_out_of_a_64_device_fleet_equals_halda_solve_batch(llama_online_model):
    devs = fleet(64, 4900)
    want = halda_solve_batch([devs[:i] + devs[i + 1:] for i in range(64)], llama_online_model)
    assert halda_leave_one_out(devs, llama_online_model) == want


def test_select_devices_drops_the_slow_device(llama_online_model):
    model = llama_online_model
    devs = fleet(8, 5000)
    slow = 5
    devs[slow] = devs[slow].model_copy(update={"t_comm": devs[slow].t_comm + 50.0})

    def brute(kept):
        """(current, the single removals) by halda_solve_batch of the sublists."""
        subs = [[devs[j] for j in kept]] + [[devs[j] for q, j in enumerate(kept) if q != i] for i in range(len(kept))]
        res = halda_solve_batch(subs, model) if len(kept) > 1 else halda_solve_batch(subs[:1], model)
        return res[0], res[1:]

    cur, rem = brute(list(range(8)))
    objs = [r.obj_value for r in rem]
    assert int(np.argmin(objs)) == slow and objs[slow] < cur.obj_value  # dropping it is the best single removal
    kept, rounds = list(range(8)), 0
    while len(kept) > 1:  # the greedy rule, every round by brute force
        cur, rem = brute(kept)
        objs = [np.inf if r is None else r.obj_value for r in rem]
        i = int(np.argmin(objs))  # the first minimum: ties to the lowest index
        if not objs[i] < cur.obj_value:
            break
        del kept[i]
        rounds += 1
    got_kept, got = halda_select_devices(devs, model)
    assert slow not in got_kept and rounds >= 1
    assert got_kept == kept
    assert got == halda_solve_batch([[devs[j] for j in kept]], model)[0]


def test_cli_leave_one_out_lines(monkeypatch, fixtures_golden):
    from distilp_amd.cli.solver import load_from_profile_folder, main

    monkeypatch.chdir(REPO)
    case = fixtures_golden["cli"]["online_default"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert main(case["argv"] + ["--leave-one-out"]) == 0
    out = buf.getvalue()
    assert out.startswith(case["stdout"])  # the normal output, unchanged
    devs, model = load_from_profile_folder("llama_3_70b/online")
    res = halda_leave_one_out(devs, model, kv_bits="4bit")
    assert all(r is not None for r in res)
    want = [f"without {d.name}: k={r.k}, obj={r.obj_value:.6f}" for d, r in zip(devs, res)]
    assert out[len(case["stdout"]):].splitlines() == want and len(want) == 2


# ---------------------------------------------------------------- reference parity
def test_leave_one_out_matches_the_recorded_reference():
    from .subfleets_cases import our_model

    G = load_json("subfleets.json")
    fleets = [our_devices(f["seed"], f["M"]) for f in G["fleets"]]
    out = halda_leave_one_out_batch(fleets, our_model(), mip_gap=G["mip_gap"], kv_bits=G["kv_bits"])
    for fl, res in zip(G["fleets"], out):
        assert len(res) == fl["M"]
        for rec, r in zip(fl["lists"], res):
            _, per_k = exact_sweep(fl["seed"], fl["M"], rec["drop"], G["kv_bits"])
            why = result_mismatch(r, rec, per_k)
            assert why is None, (fl["M"], fl["seed"], rec["drop"], why)
