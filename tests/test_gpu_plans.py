"""A deployed plan priced on the GPU (libhalda halda_eval_plans / halda_solve_fleets_plans): a sweep's own
(best_k, w, n) evaluates to the sweep's objective, the recorded and neighbour goldens evaluate as the NumPy
specification and the oracle say, the fused route (halda_sweep_plans_kernel) equals the two-launch route and
the separate calls bit for bit, and the Python entries built on them. The route is asserted in every case."""

import ctypes
import json

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import (halda_evaluate_plan, halda_evaluate_plans_batch, halda_replace_or_keep_batch,
                                halda_solve, halda_solve_batch)
from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, DeviceFleetTable, HaldaFleetResultC,
                                       HaldaPlanResultC, HaldaPlansC, _fleets_struct, fleet_table,
                                       model_struct, solve_table)
from distilp_amd.synth import synth_fleet

from .conftest import GOLDEN
from .helpers import fixture_fleet, synth_devices

pytestmark = pytest.mark.gpu

KS80 = [1, 2, 4, 5, 8, 10, 16, 20, 40]  # the default k list of the 80-layer model
SWEEP_OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c")
EVAL_OUTS = ("status", "obj_value", "cycle", "bottleneck", "reason", "x", "c")
TABLE_FIELDS = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
GUARD = 5  # entries of -7 behind every output array
KV = 0.5


def fleet(M, seed):
    return synth_devices(M, seed, synth_fleet(seed, M))


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    c.set_fleets_path("fused")
    pl.set_plans_path(c, 0)


# ------------------------------------------------------------------ self-consistency
MIXED = (1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 100)


@pytest.fixture(scope="module")
def mixed(llama_online_model):
    """Fleets over the lane and chunk boundaries, and a 240-layer copy of the model so the wide ones fit."""
    model = llama_online_model.model_copy(update={"L": 240})
    return fleet_table([fleet(M, 300 + M) for M in MIXED], model), model


@pytest.mark.parametrize("ks", [[1, 2, 3], [4, 8]])
def test_a_sweeps_own_plan_evaluates_to_its_objective(ctx, mixed, ks):
    table, model = mixed
    sizes = table.sizes()
    ctx.set_fleets_path("wave")
    wave = solve_table(table, model, ks, KV, want_x=True)
    ctx.set_fleets_path("fused")
    fused = solve_table(table, model, ks, KV, want_x=True)
    assert (wave.best_k == fused.best_k).all()
    buf = pl.evaluate_table(table, model, wave.best_k, wave.w, wave.n, KV)
    solved = wave.best_k > 0
    if ks == [4, 8]:
        assert not solved.all() and solved.any()  # W = 60 / 30: the fleets of 63 devices and more have no plan
    else:
        assert solved.all()
    for f, M in enumerate(sizes.tolist()):
        if not solved[f]:
            assert buf.status[f] == lh.STATUS_INFEASIBLE and buf.reason[f] == pl.REASON_NO_PLAN
            assert buf.obj[f] == np.inf and buf.bottleneck[f] == -1
            continue
        assert buf.status[f] == lh.STATUS_OPTIMAL and buf.reason[f] == 0, (M, buf.reason[f])
        if M <= 64:
            assert buf.obj[f] == wave.obj_value[f], (M, buf.obj[f], wave.obj_value[f])  # bit for bit
        else:
            assert rel(buf.obj[f], wave.obj_value[f]) <= 1e-12, M
        assert rel(buf.obj[f], fused.obj_value[f]) <= 1e-12, M
        j = ks.index(int(wave.best_k[f]))
        a, N = int(buf.x_off[f]), 7 * M + 1
        x, c = buf.x[a:a + N], buf.c[a:a + N]
        sx, sc = wave.x[f, j, :N], wave.c[f, j, :N]
        assert (x[:6 * M] == sx[:6 * M]).all() and x[7 * M] == sx[7 * M], M  # w, n, slacks, C
        assert (c == sc).all(), M
        assert buf.cycle[f] == x[7 * M]


# ------------------------------------------------------------------ Python bit identity
def test_evaluate_plan_equals_halda_solve_bit_for_bit(fixtures_golden, llama_online_model):
    folders = sorted({f["folder"] for f in fixtures_golden["fixtures"].values()})
    assert len(folders) == 4
    for folder in folders:
        devs, model = fixture_fleet(folder)
        for kv in ("4bit", "8bit", "fp16"):
            r = halda_solve(devs, model, plot=False, kv_bits=kv)
            e = halda_evaluate_plan(devs, model, r.k, r.w, r.n, kv)
            assert e.feasible and e.obj_value == r.obj_value, (folder, kv, e.obj_value, r.obj_value)
    for M in (1, 4, 16, 64):
        devs = fleet(M, 40 + M)
        r = halda_solve(devs, llama_online_model, plot=False, kv_bits="4bit")
        e = halda_evaluate_plan(devs, llama_online_model, r.k, r.w, r.n, "4bit")
        assert e.feasible and e.obj_value == r.obj_value, (M, e.obj_value, r.obj_value)


# ------------------------------------------------------------------ goldens
def _check_against_np(cases, model):
    """cases: (devs key, devs, k, w, n, want_success, want_obj). One batch call; every entry against the
    recorded answer and the NumPy specification."""
    evs = halda_evaluate_plans_batch([c[1] for c in cases], model, [(c[2], c[3], c[4]) for c in cases], "4bit")
    tabs = {}
    for c, e in zip(cases, evs):
        key, devs, k, w, n, ok, obj = c
        if key not in tabs:
            tabs[key] = fleet_table([devs], model)
        s = pl.evaluate_plan_np(tabs[key], model, 0, k, w, n, KV)
        assert e.feasible == ok, (key, k, e.reasons)
        if ok:
            assert rel(e.obj_value, obj) <= 1e-9, (key, k, e.obj_value, obj)
        assert e.reason == s.reason and e.status == s.status, (key, k, e.reason, s.reason)
        assert (-1 if e.bottleneck is None else e.bottleneck) == s.bottleneck, (key, k)
        assert e.cycle_time == s.cycle, (key, k, e.cycle_time, s.cycle)  # bit for bit


def test_neighbour_golden_on_the_gpu(llama_online_model):
    P = json.loads((GOLDEN / "plans.json").read_text())
    devs = {}
    cases = []
    for c in P["cases"]:
        key = (c["M"], c["seed"])
        if key not in devs:
            devs[key] = synth_devices(*key)
        cases.append((key, devs[key], c["k"], c["w"], c["n"], c["success"], c["objective_value"]))
    assert len(cases) >= 1000
    _check_against_np(cases, llama_online_model)


def test_recorded_plans_on_the_gpu(synth_golden, llama_online_model):
    cases = []
    for M in (1, 2, 3, 4, 8, 16, 32, 64):
        for fl in synth_golden[M]["fleets"]:
            devs = synth_devices(M, fl["seed"], fl["devices"])
            for rec in fl["per_k"]:
                if rec["success"]:
                    cases.append(((M, fl["seed"]), devs, rec["k"], rec["w"], rec["n"], True, rec["obj_value"]))
    assert len(cases) == 1096
    _check_against_np(cases, llama_online_model)


# ------------------------------------------------------------------ the fused route
class Run:
    """A device copy of a table, its incumbent plans, and guarded device output arrays for one call."""

    def __init__(self, table, model, ks, plan):
        torch, dev = _torch()
        self.torch, self.table, self.ks = torch, table, np.asarray(ks, np.int32)
        self.arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in TABLE_FIELDS}
        self.fs = _fleets_struct(table, lambda f: self.arrs[f].data_ptr())
        self.m = model_struct(model, KV)
        self.plan = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev) for a in plan]
        self.pc = HaldaPlansC(*[t.data_ptr() for t in self.plan])
        nf, nd, nk = table.n_fleets, table.n_devices, len(ks)
        xs = 7 * int(table.sizes().max()) + 1
        i32, f64 = torch.int32, torch.float64
        self.sizes = {"s": {"best_k": (nf, i32), "obj_value": (nf, f64), "w": (nd, i32), "n": (nd, i32),
                            "obj_by_k": (nf * nk, f64), "status": (nf * nk, i32), "x": (nf * nk * xs, f64),
                            "c": (nf * nk * xs, f64)},
                      "e": {"status": (nf, i32), "obj_value": (nf, f64), "cycle": (nf, f64), "bottleneck": (nf, i32),
                            "reason": (nf, i32), "x": (nf * xs, f64), "c": (nf * xs, f64)}}
        self.fresh()

    def fresh(self):
        torch, dev = _torch()
        self.o = {g: {f: torch.full((n + GUARD,), -7, dtype=dt, device=dev) for f, (n, dt) in d.items()}
                  for g, d in self.sizes.items()}
        self.res = HaldaFleetResultC(*[self.o["s"][f].data_ptr() for f in SWEEP_OUTS], None)
        self.eres = HaldaPlanResultC(*[self.o["e"][f].data_ptr() for f in EVAL_OUTS], None)

    def collect(self, groups=("s", "e")):
        self.torch.cuda.synchronize()
        out = {}
        for g in groups:
            for f in self.sizes[g]:
                a = self.o[g][f].cpu().numpy()
                assert (a[-GUARD:] == -7).all(), (g, f)  # the guard behind the array
                out[g + "." + f] = a[:-GUARD].copy()
        self.fresh()
        return out

    def both(self, ctx, stream=None):
        lib = ctx.lib
        rc = lib.halda_solve_fleets_plans(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs), self.ks.ctypes.data,
                                          len(self.ks), ctypes.byref(self.pc), ctypes.byref(self.eres),
                                          ctypes.byref(self.res), ctypes.c_void_p(stream) if stream else None)
        assert rc == 0, lh.last_error(lib)
        return pl.last_plans_route(ctx)

    def separate(self, ctx):
        lib = ctx.lib
        rc = lib.halda_eval_plans(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs), ctypes.byref(self.pc),
                                  ctypes.byref(self.eres), None)
        assert rc == 0, lh.last_error(lib)
        rc = lib.halda_solve_fleets(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs), self.ks.ctypes.data,
                                    len(self.ks), ctypes.byref(self.res), None)
        assert rc == 0, lh.last_error(lib)


def same(a, b):
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


def mixed_incumbents(table, model, ks):
    """Per fleet in turn: the optimum, the optimum of a re-profiled copy of the table, a plan with a layer
    too many (infeasible)."""
    opt = solve_table(table, model, ks, KV)
    per = solve_table(table.perturbed(np.random.default_rng(5), 0.8, 1.25), model, ks, KV)
    k, w, n = opt.best_k.copy(), opt.w.copy(), opt.n.copy()
    for f in range(table.n_fleets):
        a, b = int(table.dev_off[f]), int(table.dev_off[f + 1])
        if f % 3 == 1:
            k[f], w[a:b], n[a:b] = per.best_k[f], per.w[a:b], per.n[a:b]
        elif f % 3 == 2:
            w[a] += 1
    return k, w, n


@pytest.mark.parametrize("shape", ["c3", "m7"])
def test_fused_route_equals_two_launches_and_separate_calls(ctx, llama_online_model, shape):
    if shape == "c3":  # 5 fleets (not a multiple of the four waves of a workgroup) x 64 devices
        model, ks = llama_online_model, KS80
        table = fleet_table([fleet(64, 500 + s) for s in range(5)], model)
    else:  # 9 fleets x 7 devices, only k = 1 open (W = 5, 4, 2 < 7 for the others)
        model, ks = llama_online_model.model_copy(update={"L": 40}), [1, 8, 10, 20]
        table = fleet_table([fleet(7, 600 + s) for s in range(9)], model)
    run = Run(table, model, ks, mixed_incumbents(table, model, ks))
    assert run.both(ctx) == "two_launch"  # the default (the fused launch is behind path 2)
    auto = run.collect()
    pl.set_plans_path(ctx, 2)
    assert run.both(ctx) == "fused"
    fused = run.collect()
    pl.set_plans_path(ctx, 1)
    assert run.both(ctx) == "two_launch"
    two = run.collect()
    same(fused, auto)
    pl.set_plans_path(ctx, 2)
    run.separate(ctx)
    sep = run.collect()
    same(fused, two)
    same(fused, sep)
    st = fused["e.status"]
    assert (st == lh.STATUS_OPTIMAL).sum() >= 2 and (st == lh.STATUS_INFEASIBLE).any()
    assert (st[2::3] == lh.STATUS_INFEASIBLE).all() and (fused["e.reason"][2::3] & pl.REASON_SUM_W).all()
    ok = st == lh.STATUS_OPTIMAL
    assert (fused["e.obj_value"][ok] >= fused["s.obj_value"][ok]).all()  # no plan beats the optimum
    assert (fused["e.obj_value"][::3] == fused["s.obj_value"][::3]).all()  # the optimum prices as itself
    # a caller's stream against the host variant
    torch, dev = _torch()
    s = torch.cuda.Stream(dev)
    assert run.both(ctx, s.cuda_stream) == "fused"
    streamed = run.collect()
    same(fused, streamed)
    k, w, n = (t.cpu().numpy() for t in run.plan)
    res, buf = pl.solve_plans_table(table, model, list(ks), k, w, n, KV)
    assert np.array_equal(res.best_k, fused["s.best_k"]) and np.array_equal(res.obj_value, fused["s.obj_value"])
    assert np.array_equal(res.w, fused["s.w"]) and np.array_equal(res.n, fused["s.n"])
    assert np.array_equal(buf.status, fused["e.status"]) and np.array_equal(buf.obj, fused["e.obj_value"])
    assert np.array_equal(buf.cycle, fused["e.cycle"]) and np.array_equal(buf.reason, fused["e.reason"])
    assert np.array_equal(buf.bottleneck, fused["e.bottleneck"])


def test_c2_shape_takes_two_launches(ctx, llama_online_model):
    table = fleet_table([fleet(16, 700 + s) for s in range(6)], llama_online_model)
    run = Run(table, llama_online_model, KS80, mixed_incumbents(table, llama_online_model, KS80))
    pl.set_plans_path(ctx, 2)
    assert run.both(ctx) == "two_launch"  # k > 1 open: the sweep needs tables, whatever the path
    two = run.collect()
    run.separate(ctx)
    same(two, run.collect())
    assert (two["e.status"] == lh.STATUS_OPTIMAL).any() and (two["s.best_k"] > 0).all()


# ------------------------------------------------------------------ streaming
def test_resident_plan_follows_its_contents(ctx, llama_online_model):
    torch, dev = _torch()
    table = fleet_table([fleet(64, 800 + s) for s in range(6)], llama_online_model)
    dt = DeviceFleetTable(table, llama_online_model, KS80, KV, dev)
    dt.set_plans()
    pl.set_plans_path(ctx, 2)  # the incumbents ride the sweep's own launch
    s = torch.cuda.Stream(dev)
    dt.launch_with_plans(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert (dt.plan_out["reason"].cpu().numpy() == pl.REASON_NO_PLAN).all()  # none yet
    assert (dt.out["best_k"].cpu().numpy() > 0).all()
    best = dt.out["obj_value"].cpu().numpy().copy()
    with torch.cuda.stream(s):  # the new optimum becomes the incumbent, in place
        dt.plan_k.copy_(dt.out["best_k"])
        dt.plan_w.copy_(dt.out["w"])
        dt.plan_n.copy_(dt.out["n"])
        dt.plan_w[0] += 1  # but fleet 0's is broken
    dt.launch_with_plans(ctx, s.cuda_stream)
    torch.cuda.synchronize(dev)
    st, obj = dt.plan_out["status"].cpu().numpy(), dt.plan_out["obj_value"].cpu().numpy()
    assert st[0] == lh.STATUS_INFEASIBLE and (st[1:] == lh.STATUS_OPTIMAL).all()
    assert (obj[1:] == best[1:]).all() and obj[0] == np.inf
    assert (dt.out["obj_value"].cpu().numpy() == best).all()


# ------------------------------------------------------------------ API
def test_replace_or_keep_batch_equals_solve_plus_evaluate(llama_online_model):
    model = llama_online_model
    fleets = [fleet(M, 900 + M) for M in (2, 5, 16, 64)]
    old = halda_solve_batch([fleet(M, 950 + M) for M in (2, 5, 16, 64)], model, kv_bits="4bit")
    incumbents = [old[0], (old[1].k, old[1].w, old[1].n), None, old[3]]
    got = halda_replace_or_keep_batch(fleets, model, incumbents, kv_bits="4bit")
    best = halda_solve_batch(fleets, model, kv_bits="4bit")
    for f, (g, b, inc) in enumerate(zip(got, best, incumbents)):
        assert (g.best.k, g.best.w, g.best.n, g.best.obj_value) == (b.k, b.w, b.n, b.obj_value), f
        if inc is None:
            assert g.incumbent.reasons == ("no_plan",) and g.replace and g.regret == np.inf
            continue
        p = pl._as_plan(inc)
        e = halda_evaluate_plan(fleets[f], model, *p, kv_bits="4bit")
        assert g.incumbent == e, f
        if e.feasible:
            assert g.regret == e.obj_value - b.obj_value
            assert g.replace == (g.regret > 0.0)
        else:
            assert g.regret == np.inf and g.replace
        assert g.moved_layers == sum(abs(x - y) for x, y in zip(b.w, p[1]))
