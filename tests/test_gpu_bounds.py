"""The k-sweep within per-device layer bounds on the GPU (libhalda halda_solve_fleets_bounded): bounds that
never bind give halda_solve_fleets' bits on both routes, binding bounds give the exact oracle's plans, the
fused route (halda_sweep_bounds_kernel) equals the general one, wide and mixed fleets equal the host-lowered
CSR solve, the infeasible and edge cases, the DP fallback, and the Python entries. The route is asserted in
every case."""

import ctypes

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import (halda_replace_within, halda_solve, halda_solve_batch, halda_solve_bounded,
                                halda_solve_bounded_batch)
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, DeviceFleetTable, HaldaBoundsC, HaldaFleetResultC,
                                       _fleets_struct, fleet_table, model_struct, solve_table)
from distilp_amd.synth import synth_fleet

from . import bounds_cases as bc
from .helpers import fixture_fleet, synth_devices

pytestmark = pytest.mark.gpu

KS80 = [1, 2, 4, 5, 8, 10, 16, 20, 40]  # the default k list of the 80-layer model
OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c")
TABLE_FIELDS = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
GUARD = 5  # entries of -7 behind every output array
KV = bc.KV
IMAX = 2**31 - 1


def fleet(M, seed):
    return synth_devices(M, seed, synth_fleet(seed, M))


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    c.set_fleets_path("fused")
    bd.set_bounds_path(c, 0)


class Run:
    """A device copy of a table and guarded device output arrays for one call."""

    def __init__(self, table, model, ks):
        torch, dev = _torch()
        self.torch, self.dev, self.table, self.ks = torch, dev, table, np.asarray(ks, np.int32)
        self.arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in TABLE_FIELDS}
        self.fs = _fleets_struct(table, lambda f: self.arrs[f].data_ptr())
        self.m = model_struct(model, KV)
        nf, nd, nk = table.n_fleets, table.n_devices, len(ks)
        xs = 7 * int(table.sizes().max()) + 1
        i32, f64 = torch.int32, torch.float64
        self.sizes = {"best_k": (nf, i32), "obj_value": (nf, f64), "w": (nd, i32), "n": (nd, i32),
                      "obj_by_k": (nf * nk, f64), "status": (nf * nk, i32), "x": (nf * nk * xs, f64),
                      "c": (nf * nk * xs, f64)}
        self.xs = xs
        self.fresh()

    def fresh(self):
        self.o = {f: self.torch.full((n + GUARD,), -7, dtype=dt, device=self.dev) for f, (n, dt) in self.sizes.items()}
        self.res = HaldaFleetResultC(*[self.o[f].data_ptr() for f in OUTS], None)

    def collect(self):
        self.torch.cuda.synchronize()
        out = {}
        for f in self.sizes:
            a = self.o[f].cpu().numpy()
            assert (a[-GUARD:] == -7).all(), f  # the guard behind the array
            out[f] = a[:-GUARD].copy()
        self.fresh()
        return out

    def plain(self, ctx):
        lib = ctx.lib
        rc = lib.halda_solve_fleets(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs), self.ks.ctypes.data,
                                    len(self.ks), ctypes.byref(self.res), None)
        assert rc == 0, lh.last_error(lib)
        return self.collect()

    def bounded(self, ctx, w_min, w_max, null_struct=False):
        """One halda_solve_fleets_bounded call; w_min / w_max host int arrays or None (a NULL pointer)."""
        lib = ctx.lib
        keep = [None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.dev)
                for a in (w_min, w_max)]
        b = HaldaBoundsC(*[None if t is None else t.data_ptr() for t in keep])
        rc = lib.halda_solve_fleets_bounded(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs),
                                            self.ks.ctypes.data, len(self.ks), None if null_struct else ctypes.byref(b),
                                            ctypes.byref(self.res), None)
        assert rc == 0, lh.last_error(lib)
        out = self.collect()
        del keep
        return out, bd.last_bounds_route(ctx)


def same(a, b):
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


def noop_variants(table, model, ks):
    """(w_min, w_max) pairs that never bind: NULL pointers, zeros with INT32_MAX, and [1, W] for the call's
    smallest k (the largest W; for a larger k, W_k < w_max binds no more than W_k itself)."""
    nd = table.n_devices
    W = int(model.L) // min(ks)
    return [(None, None), (np.zeros(nd, np.int32), np.full(nd, IMAX, np.int32)),
            (np.ones(nd, np.int32), np.full(nd, W, np.int32)), (np.zeros(nd, np.int32), None),
            (None, np.full(nd, IMAX, np.int32))]


# ------------------------------------------------------------------ bounds that never bind
# (M, L, ks). The fused route's gate needs L - M + 1 <= 64 at k = 1 (the DP fallback's lanes), so on the
# 80-layer model only fleets of 17 devices and more pass it: the small shapes run on shorter copies of the
# model here, and on the 80-layer model itself on the general route below (SMALL_L80).
FUSED_SHAPES = {"m64": (64, 80, KS80), "m63": (63, 80, KS80), "m16": (16, 72, [1, 8, 10]), "m2": (2, 40, [1, 40]),
                "m1": (1, 40, [1])}
SMALL_L80 = {"m16": (16, [1, 8, 10]), "m2": (2, [1, 80]), "m1": (1, [1])}


def shape_model(model, L):
    return model if L == int(model.L) else model.model_copy(update={"L": L})


@pytest.mark.parametrize("shape", sorted(FUSED_SHAPES))
def test_noop_bounds_equal_the_sweep_on_the_fused_route(ctx, llama_online_model, shape):
    M, L, ks = FUSED_SHAPES[shape]
    model = shape_model(llama_online_model, L)
    table = fleet_table([fleet(M, 1100 + s) for s in range(5)], model)
    run = Run(table, model, ks)
    want = run.plain(ctx)
    assert (want["best_k"] > 0).all()
    got, route = run.bounded(ctx, None, None, null_struct=True)
    assert route == "fused"
    same(got, want)
    for lo, hi in noop_variants(table, model, ks):
        got, route = run.bounded(ctx, lo, hi)
        assert route == "fused", shape
        same(got, want)
    bd.set_bounds_path(ctx, 2)
    got, route = run.bounded(ctx, None, None)
    assert route == "fused"
    same(got, want)


@pytest.mark.parametrize("shape", sorted(SMALL_L80))
def test_noop_bounds_on_small_fleets_of_the_80_layer_model(ctx, llama_online_model, shape):
    """L - M + 1 > 64 at k = 1: not the fused route's gate, so the general route, whose outputs are the CSR
    pipeline's bit for bit and the default sweep's plans (objectives within the cross-path bound)."""
    M, ks = SMALL_L80[shape]
    model = llama_online_model
    table = fleet_table([fleet(M, 1100 + s) for s in range(5)], model)
    run = Run(table, model, ks)
    sweep = run.plain(ctx)
    ctx.set_fleets_path("csr")
    want = run.plain(ctx)
    ctx.set_fleets_path("fused")
    for lo, hi in noop_variants(table, model, ks):
        got, route = run.bounded(ctx, lo, hi)
        assert route == "general", shape
        same(got, want)
    for f in ("best_k", "w", "n", "status"):
        assert np.array_equal(got[f], sweep[f]), f
    assert (sweep["best_k"] > 0).all()
    assert (np.abs(got["obj_value"] - sweep["obj_value"]) <= 1e-12 * np.abs(sweep["obj_value"])).all()


MIXED = (1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 100)


@pytest.fixture(scope="module")
def mixed(llama_online_model):
    """Fleets over the lane and chunk boundaries, and a 240-layer copy of the model so the wide ones fit."""
    model = llama_online_model.model_copy(update={"L": 240})
    return fleet_table([fleet(M, 300 + M) for M in MIXED], model), model


@pytest.mark.parametrize("ks", [[1, 2, 3], [4, 8]])
def test_noop_bounds_equal_the_csr_pipeline_on_the_general_route(ctx, mixed, ks):
    table, model = mixed
    run = Run(table, model, ks)
    ctx.set_fleets_path("csr")  # halda_solve_fleets through the pipeline the general route reuses
    want = run.plain(ctx)
    ctx.set_fleets_path("fused")
    for lo, hi in noop_variants(table, model, ks):
        got, route = run.bounded(ctx, lo, hi)
        assert route == "general"
        same(got, want)
    # and against the fused sweep: the plans, and the objectives within the cross-path bound
    sweep = run.plain(ctx)
    for f in ("best_k", "w", "n", "status"):
        assert np.array_equal(got[f], sweep[f]), f
    ok = sweep["best_k"] > 0
    assert (np.abs(got["obj_value"][ok] - sweep["obj_value"][ok]) <= 1e-12 * np.abs(sweep["obj_value"][ok])).all()


# ------------------------------------------------------------------ binding bounds against the exact oracle
def check_against_oracle(ctx, model, M, k, want_route):
    """The 12 fleets x (D = 1, D = 2, uniform cap) cases of (M, k) in ONE call; every case against the exact
    oracle: status, (w, n), c.x and the objective."""
    cs = bc.cases([M], [k])
    devs = [list(bc.devices(M, s)) for _, _, s, _ in cs]
    boxes = [bc.box(model, M, k, s, kind) for _, _, s, kind in cs]
    table = fleet_table(devs, model)
    lo, hi = bc.flat(boxes, table)
    run = Run(table, model, [k])
    got, route = run.bounded(ctx, lo, hi)
    assert route == want_route
    free = run.plain(ctx)
    N, differ = 7 * M + 1, 0
    for f, (c, dv, (blo, bhi)) in enumerate(zip(cs, devs, boxes)):
        st, w, n, cx, obj, unique = bc.exact_answer(model, dv, k, blo, bhi)
        assert st == 0 and unique, c  # every case is feasible and unique: none is skipped
        assert got["status"][f] == lh.STATUS_OPTIMAL and got["best_k"][f] == k, c
        a = f * M
        assert got["w"][a:a + M].tolist() == w and got["n"][a:a + M].tolist() == n, c
        assert all(l <= v <= h for l, v, h in zip(blo, w, bhi)), c
        x, cc = got["x"][f * run.xs:f * run.xs + N], got["c"][f * run.xs:f * run.xs + N]
        assert bc.rel(float(cc.dot(x)), cx) <= 1e-9, c
        assert bc.rel(got["obj_value"][f], obj) <= 1e-9 and got["obj_by_k"][f] == got["obj_value"][f], c
        differ += got["w"][a:a + M].tolist() != free["w"][a:a + M].tolist()
    return differ, len(cs)


def test_binding_bounds_on_the_fused_route_equal_the_oracle(ctx, llama_online_model):
    differ, total = check_against_oracle(ctx, llama_online_model, 64, 1, "fused")
    assert total == 36 and differ >= 24  # the bounds bind: most plans differ from the unbounded optimum


@pytest.mark.parametrize("M", [4, 8, 16])
@pytest.mark.parametrize("k", [1, 2, 4, 5])
def test_binding_bounds_on_the_general_route_equal_the_oracle(ctx, llama_online_model, M, k):
    differ, total = check_against_oracle(ctx, llama_online_model, M, k, "general")
    assert total == 36
    if not (M == 16 and k == 5):  # W = M there: the plan is forced
        assert differ >= 18


# ------------------------------------------------------------------ fused equals general
def fused_inputs(model80):
    """The fused-route inputs: the no-op shapes with their binding boxes (D = 2 around another seed's k = 1
    optimum, every third device not allowed to grow)."""
    out = []
    for shape in sorted(FUSED_SHAPES):
        M, L, ks = FUSED_SHAPES[shape]
        model = shape_model(model80, L)
        devs = [fleet(M, 1100 + s) for s in range(5)]
        table = fleet_table(devs, model)
        inc = solve_table(fleet_table([fleet(M, 1200 + s) for s in range(5)], model), model, [1], KV)
        W = int(model.L)
        lo = np.maximum(1, inc.w - 2).astype(np.int32)
        hi = np.minimum(W, inc.w + 2).astype(np.int32)
        hi[::3] = np.maximum(inc.w[::3], 1)  # every third device may not grow
        out.append((shape, table, model, ks, lo, np.maximum(hi, lo)))
    return out


def test_fused_route_equals_the_general_route(ctx, llama_online_model):
    for shape, table, model, ks, lo, hi in fused_inputs(llama_online_model):
        run = Run(table, model, ks)
        bd.set_bounds_path(ctx, 0)
        fused, route = run.bounded(ctx, lo, hi)
        assert route == "fused", shape
        bd.set_bounds_path(ctx, 1)
        gen, route = run.bounded(ctx, lo, hi)
        assert route == "general", shape
        for f in ("status", "best_k", "w", "n"):
            assert np.array_equal(fused[f], gen[f]), (shape, f)
        for f in ("obj_value", "obj_by_k"):
            a, b = fused[f], gen[f]
            fin = np.isfinite(b)
            assert np.array_equal(np.isfinite(a), fin), (shape, f)
            assert (np.abs(a[fin] - b[fin]) <= 1e-12 * np.maximum(1.0, np.abs(b[fin]))).all(), (shape, f)
        assert (fused["best_k"] == 1).all(), shape  # the box around a feasible plan holds one


def test_dp_fallback_gives_the_greedys_outputs(ctx, llama_online_model):
    for shape, table, model, ks, lo, hi in fused_inputs(llama_online_model):
        run = Run(table, model, ks)
        greedy, route = run.bounded(ctx, lo, hi)
        assert route == "fused"
        ctx.set_fleets_path("dp")
        dp, route = run.bounded(ctx, lo, hi)
        ctx.set_fleets_path("fused")
        assert route == "fused", shape
        same(dp, greedy)


# ------------------------------------------------------------------ wide and mixed fleets: the host-lowered CSR
def test_wide_and_mixed_fleets_equal_the_patched_host_lowering(ctx, mixed):
    """The general route against the milp() replacement's entry (halda_solve_batch on a host CSR): the host
    lowering of each (fleet, k) with its w column bounds patched in NumPy."""
    from distilp_amd.solver.batch import assemble
    from distilp_amd.solver.lower import lower_fleet

    table, model = mixed
    ks = [1, 2, 3]
    rng = np.random.default_rng(11)
    free = solve_table(table, model, ks, KV)
    lo = np.maximum(1, free.w - rng.integers(0, 3, table.n_devices)).astype(np.int32)
    hi = np.minimum(int(model.L), free.w + rng.integers(0, 3, table.n_devices)).astype(np.int32)
    run = Run(table, model, ks)
    got, route = run.bounded(ctx, lo, hi)
    assert route == "general"
    milps = [lower_fleet(fleet(M, 300 + M), model, kv_factor=KV) for M in MIXED]
    batch, refs = assemble(milps, [ks] * len(MIXED), mip_gap=0.0)
    for r in refs:
        M, a = MIXED[r.fleet], int(table.dev_off[r.fleet])
        batch.col_lb[r.col_off:r.col_off + M] = lo[a:a + M]
        batch.col_ub[r.col_off:r.col_off + M] = np.minimum(hi[a:a + M], r.W)
    want = ctx.solve(batch)
    for q, r in enumerate(refs):
        M, N = MIXED[r.fleet], r.n_cols
        assert got["status"][q] == want.status[q], (M, r.k)
        if want.status[q] != lh.STATUS_OPTIMAL:
            continue
        x = got["x"][q * run.xs:q * run.xs + N]
        assert np.array_equal(x, want.x[r.col_off:r.col_off + N]), (M, r.k)
        cx = float(got["c"][q * run.xs:q * run.xs + N].dot(x))
        assert bc.rel(cx, want.obj_lin[q]) <= 1e-12, (M, r.k)
        a = int(table.dev_off[r.fleet])
        assert (x[:M] >= lo[a:a + M]).all() and (x[:M] <= hi[a:a + M]).all(), (M, r.k)
    assert (got["status"] == lh.STATUS_OPTIMAL).sum() >= len(MIXED)


# ------------------------------------------------------------------ infeasible and edge cases, both routes
@pytest.mark.parametrize("path", [0, 1])
def test_infeasible_and_edge_cases(ctx, llama_online_model, path):
    model = llama_online_model
    M, ks, W = 64, KS80, 80
    devs = [fleet(M, 1300 + s) for s in range(7)]
    table = fleet_table(devs, model)
    run = Run(table, model, ks)
    bd.set_bounds_path(ctx, path)
    want_route = "fused" if path == 0 else "general"
    free = run.plain(ctx)
    w0 = free["w"].reshape(7, M)
    lo, hi = np.ones((7, M), np.int32), np.full((7, M), IMAX, np.int32)
    hi[0, :] = 1                      # fleet 0: sum hi = 64 < W
    lo[1, :] = 2                      # fleet 1: sum lo = 128 > W
    lo[2, 5], hi[2, 5] = 4, 3         # fleet 2: one device with lo > hi
    lo[3, :] = 1
    lo[3, :16] = 2                    # fleet 3: sum lo = 80 = W, the plan is forced
    lo[4, :] = hi[4, :] = w0[4]       # fleet 4: every device pinned at the free optimum
    lo[5, 7] = hi[5, 7] = w0[5, 7] + 2  # fleet 5: one device pinned two layers above its optimum
    # fleet 6: no bounds
    got, route = run.bounded(ctx, lo.ravel(), hi.ravel())
    assert route == want_route
    st = got["status"].reshape(7, len(ks))
    assert (st[:3] == lh.STATUS_INFEASIBLE).all() and (got["best_k"][:3] == 0).all()
    assert (got["obj_value"][:3] == np.inf).all() and (got["w"].reshape(7, M)[:3] == 0).all()
    assert (st[3:, 0] == lh.STATUS_OPTIMAL).all() and (st[3:, 1:] == lh.STATUS_INFEASIBLE).all()
    w, n = got["w"].reshape(7, M), got["n"].reshape(7, M)
    assert w[3].tolist() == [2] * 16 + [1] * 48
    assert np.array_equal(w[4], w0[4]) and np.array_equal(n[4], free["n"].reshape(7, M)[4])
    assert w[5, 7] == w0[5, 7] + 2 and w[5].sum() == W and got["obj_value"][5] > free["obj_value"][5]
    assert np.array_equal(w[6], w0[6])
    if path == 0:
        assert got["obj_value"][4] == free["obj_value"][4] and got["obj_value"][6] == free["obj_value"][6]
    else:
        assert bc.rel(got["obj_value"][4], free["obj_value"][4]) <= 1e-12
    # the forced and the pinned plans against the exact oracle
    for f in (3, 5):
        s_, ow, on, _, obj, _ = bc.exact_answer(model, devs[f], 1, lo[f].tolist(), np.minimum(hi[f], W).tolist())
        assert s_ == 0 and w[f].tolist() == ow and n[f].tolist() == on and bc.rel(got["obj_value"][f], obj) <= 1e-9
    # every returned (k, w, n) priced by halda_eval_plans: the same obj_value, bit for bit on the fused route
    buf = pl.evaluate_table(table, model, got["best_k"], got["w"], got["n"], KV)
    for f in range(3, 7):
        assert buf.status[f] == lh.STATUS_OPTIMAL
        if path == 0:
            assert buf.obj[f] == got["obj_value"][f], f
        else:
            assert bc.rel(buf.obj[f], got["obj_value"][f]) <= 1e-12, f


# ------------------------------------------------------------------ the Python entries
def test_solve_bounded_without_bounds_equals_halda_solve(fixtures_golden):
    folders = sorted({f["folder"] for f in fixtures_golden["fixtures"].values()})
    assert len(folders) == 4
    for folder in folders:
        devs, model = fixture_fleet(folder)
        r = halda_solve(devs, model, plot=False, kv_bits="4bit")
        for kw in ({}, {"w_min": [1] * len(devs)}, {"w_max": [int(model.L)] * len(devs)}):
            b = halda_solve_bounded(devs, model, kv_bits="4bit", **kw)
            assert (b.k, b.w, b.n, b.obj_value, b.sets) == (r.k, r.w, r.n, r.obj_value, r.sets), (folder, kw)


def test_replace_within_on_a_reprofiled_fleet(llama_online_model):
    model = llama_online_model
    for M in (4, 16, 64):
        devs = fleet(M, 1400 + M)
        inc = halda_solve(fleet(M, 1500 + M), model, plot=False, kv_bits="4bit", k_candidates=[1])
        for D in (1, 2):
            r = halda_replace_within(devs, model, inc, D, kv_bits="4bit")
            lo, hi = bd.move_bounds(inc.w, D)
            assert r.within is not None and r.within.k == inc.k
            assert all(l <= v <= h for l, v, h in zip(lo, r.within.w, hi)) and sum(r.within.w) == model.L
            assert r.gap_to_free >= 0.0 and r.moved_layers_within <= D * M
            assert r.moved_layers_within == sum(abs(a - b) for a, b in zip(r.within.w, inc.w))
            if r.incumbent.feasible:
                assert r.regret_within == r.incumbent.obj_value - r.within.obj_value and r.regret_within >= 0.0
        big = halda_replace_within(devs, model, inc, int(model.L), kv_bits="4bit")
        free = halda_solve_batch([devs], model, k_candidates=[inc.k], kv_bits="4bit")[0]
        assert (big.within.w, big.within.n, big.within.obj_value) == (free.w, free.n, free.obj_value), M


def test_bounded_batch_mixes_bounded_and_free_fleets(llama_online_model):
    model = llama_online_model
    fleets = [fleet(M, 1600 + M) for M in (3, 8, 8, 20)]
    free = halda_solve_batch(fleets, model, k_candidates=[1, 10], kv_bits="4bit")
    free1 = halda_solve_batch(fleets[1:2], model, k_candidates=[1], kv_bits="4bit")[0]
    i = int(np.argmax(free1.w))  # fleet 1: its largest k = 1 share capped one layer lower
    hi1 = [80] * 8
    hi1[i] = free1.w[i] - 1
    cap = [None, ([1] * 8, hi1), ([1] * 8, [1] * 8), None]
    got = halda_solve_bounded_batch(fleets, model, cap, k_candidates=[1, 10], kv_bits="4bit")
    assert (got[0].w, got[0].obj_value) == (free[0].w, free[0].obj_value)
    assert (got[3].w, got[3].obj_value) == (free[3].w, free[3].obj_value)
    assert got[1].w[i] <= hi1[i] and got[1].obj_value >= free[1].obj_value
    assert got[2].w == [1] * 8 and got[2].k == 10  # every device capped at one layer: only W = 8 fits
    with pytest.raises(RuntimeError, match="No feasible MILP"):
        halda_solve_bounded(fleets[2], model, w_max=[1] * 8, k_candidates=[1], kv_bits="4bit")


def test_resident_bounds_follow_their_contents(ctx, llama_online_model):
    torch, dev = _torch()
    model = llama_online_model
    table = fleet_table([fleet(64, 1700 + s) for s in range(6)], model)
    dt = DeviceFleetTable(table, model, KS80, KV, dev)
    dt.set_bounds()
    s = torch.cuda.Stream(dev)
    dt.launch_with_bounds(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert bd.last_bounds_route(ctx) == "fused"
    w0, best = dt.out["w"].cpu().numpy().copy(), dt.out["obj_value"].cpu().numpy().copy()
    dt.launch(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(dt.out["w"].cpu().numpy(), w0) and np.array_equal(dt.out["obj_value"].cpu().numpy(), best)
    with torch.cuda.stream(s):  # in place: fleet 0 pinned at its optimum, fleet 1's first device one layer lower
        dt.bound_min[:64].copy_(dt.out["w"][:64])
        dt.bound_max[:64].copy_(dt.out["w"][:64])
        dt.bound_max[64] = int(w0[64]) - 1 if w0[64] > 1 else IMAX
    dt.launch_with_bounds(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    w1, obj1 = dt.out["w"].cpu().numpy(), dt.out["obj_value"].cpu().numpy()
    assert np.array_equal(w1[:64], w0[:64]) and obj1[0] == best[0]
    if w0[64] > 1:
        assert w1[64] <= w0[64] - 1 and obj1[1] >= best[1]
    assert np.array_equal(w1[128:], w0[128:]) and np.array_equal(obj1[2:], best[2:])
