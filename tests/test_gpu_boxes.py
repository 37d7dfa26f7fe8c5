"""One fleet table under many boxes on the GPU (libhalda halda_solve_fleets_boxes): slice b of every output equals,
bit for bit, the single-box halda_solve_fleets_boxed_host call under bounds path 3, on the register route
(halda_sweep_boxes_kernel), the table route (halda_sweep_boxes_tables_kernel) and the loop route; the loop test
path gives the fused routes' bits; a NULL array is its "no bound" fill; the slices equal the exact oracle; the
argument errors launch nothing; and the reload-time frontier built on the call (halda_reload_frontier) and its CLI
lines. The route is asserted in every case."""

import contextlib
import ctypes
import io
import re

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import boxes as bx
from distilp_amd.solver import halda_reload_frontier, halda_solve_bounded, halda_solve_boxes
from distilp_amd.solver._abi import HaldaBoxC, HaldaBoxesC, HaldaFleetResultC
from distilp_amd.solver.fleets import _host_struct, fleet_table, model_struct, open_x_offsets

from . import bounds_cases as bc
from . import box_cases as xc
from . import budget_cases as gc
from .conftest import REPO
from .test_boxes import RELOAD_CASES

pytestmark = pytest.mark.gpu

KV = bc.KV
IMAX = 2**31 - 1
KS80 = [1, 2, 4, 5, 8, 10, 16, 20, 40]  # the default k list of the 80-layer model
FILL = (0, IMAX, 0, IMAX)  # the "no bound" value of w_min, w_max, n_min, n_max
GUARD = 5  # entries of -7 behind every output array
E_ARG = -22


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    bd.set_bounds_path(c, 0)
    bx.set_boxes_path(c, 0)


class Host:
    """A packed table with the compact x / c layout of one box, and guarded host output arrays for `rows` boxes."""

    def __init__(self, table, model, ks):
        self.table, self.ks = table, np.asarray(ks, np.int32)
        self.m = model_struct(model, KV)
        self.fs, self.keep = _host_struct(table)
        self.nf, self.nd, self.nk = table.n_fleets, table.n_devices, len(ks)
        self.xsel = open_x_offsets(table, model, list(ks))
        open_ = self.xsel >= 0
        self.ext = int(np.max(self.xsel + np.repeat(7 * table.sizes() + 1, self.nk), initial=0)) if open_.any() else 0

    def outputs(self, nb):
        nf, nd, nk = self.nf, self.nd, self.nk
        sizes = {"best_k": (nb * nf, np.int32), "obj_value": (nb * nf, np.float64), "w": (nb * nd, np.int32),
                 "n": (nb * nd, np.int32), "obj_by_k": (nb * nf * nk, np.float64), "status": (nb * nf * nk, np.int32),
                 "x": (nb * self.ext, np.float64), "c": (nb * self.ext, np.float64)}
        o = {f: np.full(n + GUARD, -7, dt) for f, (n, dt) in sizes.items()}
        base = (np.arange(nb, dtype=np.int64) * self.ext)[:, None]
        x_off = np.where(self.xsel[None, :] >= 0, self.xsel[None, :] + base, -1).astype(np.int64).ravel()
        res = HaldaFleetResultC(*[o[f].ctypes.data for f in ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x",
                                                             "c")], x_off.ctypes.data)
        return o, res, x_off

    @staticmethod
    def collect(o, nb):
        """Per output an [nb, ...] array of raw 32- or 64-bit words (a double is compared by its bits)."""
        out = {}
        for f, a in o.items():
            assert (a[-GUARD:] == -7).all(), f  # the guard behind the array
            out[f] = a[:-GUARD].view(np.uint64 if a.dtype == np.float64 else np.int32).reshape(nb, -1).copy()
        return out

    def boxes(self, ctx, planes, nb, want_rc=0):
        """One halda_solve_fleets_boxes_host call; planes: four [nb, nd] int arrays or None (a NULL pointer) each."""
        keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in planes]
        assert all(a is None or a.shape == (max(nb, 0), self.nd) or want_rc for a in keep)
        o, res, x_off = self.outputs(max(nb, 1) if want_rc else nb)
        b = HaldaBoxesC(nb, *[lh.ptr(a) for a in keep])
        rc = ctx.lib.halda_solve_fleets_boxes_host(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs),
                                                   self.ks.ctypes.data, self.nk, ctypes.byref(b), ctypes.byref(res))
        assert rc == want_rc, lh.last_error(ctx.lib)
        if want_rc:
            return o
        return self.collect(o, nb), bx.last_boxes_route(ctx)

    def boxed(self, ctx, box):
        """One halda_solve_fleets_boxed_host call under bounds path 3; box: four [nd] int arrays or None each."""
        keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in box]
        o, res, x_off = self.outputs(1)
        b = HaldaBoxC(*[lh.ptr(a) for a in keep])
        bd.set_bounds_path(ctx, 3)
        rc = ctx.lib.halda_solve_fleets_boxed_host(ctx.ctx, ctypes.byref(self.m), ctypes.byref(self.fs),
                                                   self.ks.ctypes.data, self.nk, ctypes.byref(b), ctypes.byref(res))
        bd.set_bounds_path(ctx, 0)
        assert rc == 0, lh.last_error(ctx.lib)
        return self.collect(o, 1), bd.last_bounds_route(ctx)


def same(a, b, what=None):
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(a[f], b[f]), (what, f)


def slice_of(out, b):
    return {f: a[b:b + 1] for f, a in out.items()}


def kind_box(model, fleets, k, kind):
    """One box over the fleets [(M, seed)]: box_cases.box of the kind per fleet (the fill where it has no case),
    "none" (no bound anywhere), "nmax" (only n_max: half of W on every device) or ("cap", c) (w_max = c)."""
    W = int(model.L) // k
    rows = [[], [], [], []]
    for M, s in fleets:
        if kind == "none":
            b = None
        elif kind == "nmax":
            b = ([FILL[0]] * M, [FILL[1]] * M, [FILL[2]] * M, [W // 2] * M)
        elif isinstance(kind, tuple):
            b = ([FILL[0]] * M, [kind[1]] * M, [FILL[2]] * M, [FILL[3]] * M)
        else:
            b = xc.box(model, M, k, s, kind)
        for a in range(4):
            rows[a] += [FILL[a]] * M if b is None else list(b[a])
    return [np.asarray(r, np.int64).clip(-IMAX, IMAX).astype(np.int32) for r in rows]


def planes_of(model, fleets, k, kinds):
    per = [kind_box(model, fleets, k, kind) for kind in kinds]
    return [np.stack([p[a] for p in per]) for a in range(4)]


ALL_KINDS = xc.KINDS + ("none", "nmax")
# name -> (route, [(M, seed)], ks, the k the boxes are built at, kinds)
SHAPES = {
    # five fleets: not a multiple of the four waves per workgroup
    "reg-5x24": ("register", [(24, s) for s in range(5)], [1], 1, ALL_KINDS),
    "reg-3x64": ("register", [(64, s) for s in range(3)], KS80, 1, ALL_KINDS),
    # mixed sizes: an odd device count, so the b * nd offsets are odd too
    "tab-mixed": ("tables", [(1, 0), (3, 1), (7, 2), (16, 3), (16, 4)], [1, 2, 4, 5], 2, ALL_KINDS),
    "tab-1x16": ("tables", [(16, 5)], [2], 2, ALL_KINDS + (("cap", 4), ("cap", 6), ("cap", 9))),
    "loop-2x70": ("loop", [(70, 0), (70, 1)], [1, 2], 1, ("box1", "off", "none")),
}
_RUNS = {}


def shape_run(model, name):
    """(Host, planes, n_box) of a shape, built once."""
    if name not in _RUNS:
        _, fleets, ks, k, kinds = SHAPES[name]
        table = fleet_table([list(bc.devices(M, s)) for M, s in fleets], model)
        _RUNS[name] = (Host(table, model, ks), planes_of(model, fleets, k, kinds), len(kinds))
    return _RUNS[name]


# ------------------------------------------------------------------ 1. bits: every slice is the single-box call
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_slice_equals_the_single_box_call(ctx, llama_online_model, name):
    route = SHAPES[name][0]
    run, planes, nb = shape_run(llama_online_model, name)
    if name == "tab-mixed":
        assert run.nd % 2 == 1
    if name == "tab-1x16":
        assert nb == 12
    got, r = run.boxes(ctx, planes, nb)
    assert r == route, name
    single = {"register": "fused", "tables": "tables", "loop": "general"}[route]
    solved = 0
    for b in range(nb):
        want, rb = run.boxed(ctx, [p[b] for p in planes])
        assert rb == single, (name, b)
        same(slice_of(got, b), want, (name, b))
        solved += int((want["best_k"] > 0).sum())
    assert solved >= nb * run.nf // 2  # most boxes hold a plan: the comparison is not of zeros
    # n_box = 1 is the boxed call
    one, r = run.boxes(ctx, [p[:1] for p in planes], 1)
    assert r == route
    same(one, slice_of(got, 0), name)


@pytest.mark.parametrize("name", ["reg-5x24", "tab-mixed"])
def test_a_null_array_is_its_no_bound_fill(ctx, llama_online_model, name):
    route = SHAPES[name][0]
    run, planes, nb = shape_run(llama_online_model, name)
    for a in range(4):
        null = [None if i == a else p for i, p in enumerate(planes)]
        fill = [np.full_like(p, FILL[a]) if i == a else p for i, p in enumerate(planes)]
        got, r = run.boxes(ctx, null, nb)
        want, r2 = run.boxes(ctx, fill, nb)
        assert r == r2 == route
        same(got, want, (name, a))
    # no n array at all: the bounded records; fills that never bind give the same bits
    got, r = run.boxes(ctx, [planes[0], planes[1], None, None], nb)
    want, _ = run.boxes(ctx, [planes[0], planes[1], np.full_like(planes[2], FILL[2]), np.full_like(planes[3], FILL[3])],
                        nb)
    assert r == route
    same(got, want, name)


# ------------------------------------------------------------------ 2. the loop test path
@pytest.mark.parametrize("name", ["reg-5x24", "reg-3x64", "tab-mixed", "tab-1x16"])
def test_loop_path_gives_the_fused_routes_bits(ctx, llama_online_model, name):
    route = SHAPES[name][0]
    run, planes, nb = shape_run(llama_online_model, name)
    auto, r = run.boxes(ctx, planes, nb)
    assert r == route
    bd.set_bounds_path(ctx, 1)  # the caller's own bounds path: the loop runs under path 3 and puts this one back
    bx.set_boxes_path(ctx, 1)
    loop, r = run.boxes(ctx, planes, nb)
    assert r == "loop"
    assert bd.last_bounds_route(ctx) == {"register": "fused", "tables": "tables"}[route]
    same(loop, auto, name)
    bx.set_boxes_path(ctx, 0)
    # the context's bounds path is still the caller's: a boxed call now takes the general route
    o, res, _ = run.outputs(1)
    b = HaldaBoxC(*[lh.ptr(np.ascontiguousarray(p[0])) for p in planes])
    rc = ctx.lib.halda_solve_fleets_boxed_host(ctx.ctx, ctypes.byref(run.m), ctypes.byref(run.fs), run.ks.ctypes.data,
                                               run.nk, ctypes.byref(b), ctypes.byref(res))
    assert rc == 0 and bd.last_bounds_route(ctx) == "general"


# ------------------------------------------------------------------ 3. the slices against the exact oracle
ORACLE_KINDS = ("box1", "box2", "off", "half", "pin", "cross")


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("k", [1, 2])
def test_slices_equal_the_exact_oracle(ctx, llama_online_model, M, k):
    model = llama_online_model
    fleets = [(M, s) for s in range(3)]
    table = fleet_table([list(bc.devices(M, s)) for M, s in fleets], model)
    run = Host(table, model, [k])
    planes = planes_of(model, fleets, k, ORACLE_KINDS)
    got, r = run.boxes(ctx, planes, len(ORACLE_KINDS))
    assert r == "tables"
    W = int(model.L) // k
    feasible = unique_plans = 0
    for b, kind in enumerate(ORACLE_KINDS):
        for f, (_, s) in enumerate(fleets):
            a = f * M
            box = [p[b, a:a + M].tolist() for p in planes]
            box[0] = [max(1, v) for v in box[0]]
            box[1] = [min(W, v) for v in box[1]]
            st, x, _, obj, unique = xc.exact_answer(model, list(bc.devices(M, s)), k, box)
            case = (M, k, s, kind)
            if st != 0:
                assert got["status"][b, f] == lh.STATUS_INFEASIBLE and got["best_k"][b, f] == 0, case
                continue
            feasible += 1
            assert got["status"][b, f] == lh.STATUS_OPTIMAL and got["best_k"][b, f] == k, case
            assert bc.rel(float(got["obj_value"][b, f:f + 1].view(np.float64)[0]), obj) <= 1e-9, case
            if unique:
                unique_plans += 1
                assert got["w"][b, a:a + M].tolist() == [int(round(v)) for v in x[:M]], case
                assert got["n"][b, a:a + M].tolist() == [int(round(v)) for v in x[M:2 * M]], case
    assert feasible >= 9 and unique_plans >= feasible // 2


# ------------------------------------------------------------------ 4. the argument errors launch nothing
def test_a_bad_box_count_is_an_argument_error(ctx, llama_online_model):
    run, planes, nb = shape_run(llama_online_model, "reg-5x24")
    _, before = run.boxes(ctx, planes, nb)
    for bad in (0, 65536, -1):
        o = run.boxes(ctx, planes, bad, want_rc=E_ARG)
        assert "n_box" in lh.last_error(ctx.lib)
        assert all((a == -7).all() for a in o.values())  # nothing was written
        assert bx.last_boxes_route(ctx) == before
    # the device entry checks the count before it touches a pointer
    b = HaldaBoxesC(0, None, None, None, None)
    res = HaldaFleetResultC(*[None] * 9)
    rc = ctx.lib.halda_solve_fleets_boxes(ctx.ctx, ctypes.byref(run.m), ctypes.byref(run.fs), run.ks.ctypes.data, run.nk,
                                          ctypes.byref(b), ctypes.byref(res), None)
    assert rc == E_ARG
    with pytest.raises(RuntimeError):
        bx.set_boxes_path(ctx, 2)


# ------------------------------------------------------------------ 5. the Python entries
def test_solve_boxes_equals_the_bounded_batch(llama_online_model):
    model = llama_online_model
    fleets = [list(bc.devices(M, s)) for M, s in ((3, 1), (8, 2), (24, 3))]
    n_max = [IMAX] * 8
    n_max[0] = 0
    boxes = [[None, None, None], [(None, [40, 30, 20]), ([2] * 8, None), None],
             [None, (None, None, None, n_max), ([1] * 24, [5] * 24)], [([30, 30, 30], None), None, None]]
    got = bx.halda_solve_boxes_batch(fleets, model, boxes, [1, 2, 4], kv_bits="4bit")
    assert bx.last_boxes_route(lh.get_context(0)) == "tables"
    for b, box in enumerate(boxes):
        want = bd.halda_solve_bounded_batch(fleets, model, box, [1, 2, 4], kv_bits="4bit", route="tables")
        for f, (g, w) in enumerate(zip(got[b], want)):
            assert (g is None) == (w is None), (b, f)
            if g is not None:
                assert (g.k, g.w, g.n, g.obj_value, g.sets) == (w.k, w.w, w.n, w.obj_value, w.sets), (b, f)
    assert got[3][0] is None and got[0][0] is not None  # sum w_min = 90 > 80
    one = halda_solve_boxes(fleets[1], model, [b[1] for b in boxes], [1, 2, 4], kv_bits="4bit")
    assert [(r.k, r.w, r.n, r.obj_value) for r in one] == [(r[1].k, r[1].w, r[1].n, r[1].obj_value) for r in got]


# ------------------------------------------------------------------ 6. the reload-time frontier
def result_key(r):
    return None if r is None else (r.k, list(r.w), list(r.n), r.obj_value)


@pytest.mark.parametrize("M,k,s", RELOAD_CASES)
def test_reload_frontier(llama_online_model, M, k, s):
    model = llama_online_model
    devs, w0 = gc.list_case(model, M, k, s)
    inc = (k, w0, [0] * M)
    group = float(k * int(model.b_layer))
    sd = [float(d.s_disk) for d in devs]
    # a short ladder, every point against its own bounded solve, before the running minimum
    pts = halda_reload_frontier(devs, model, inc, max_points=24, kv_bits="4bit")
    assert len(pts) == 24
    raw = halda_solve_boxes(devs, model, [(None, [a + c for a, c in zip(w0, p.caps)]) for p in pts], [k],
                            kv_bits="4bit")
    best = None
    for j, (p, r) in enumerate(zip(pts, raw)):
        want = halda_solve_bounded(devs, model, w_max=[a + c for a, c in zip(w0, p.caps)], k_candidates=[k],
                                   kv_bits="4bit", route="tables")
        assert result_key(r) == result_key(want), (M, k, s, j)
        if best is None or r.obj_value < best.obj_value:
            best = r
        assert result_key(p.plan) == result_key(best) and p.obj_value == best.obj_value, (M, k, s, j)
    assert pts[0].plan.w == w0 and pts[0].seconds == 0.0 and pts[0].caps == [0] * M
    # the whole ladder
    full = halda_reload_frontier(devs, model, inc, max_points=4096, kv_bits="4bit")
    t, caps = bx.reload_caps(w0, sd, int(model.L) // k, max_points=4096)
    assert len(full) == len(t) > 24 and [p.caps for p in full] == caps.tolist()
    assert [p.seconds for p in full] == [float(v) * group for v in t]
    assert [result_key(p.plan) for p in full[:24]] == [result_key(p.plan) for p in pts]
    objs = [p.obj_value for p in full]
    assert all(b <= a for a, b in zip(objs, objs[1:]))
    assert full[0].plan.w == w0 and full[0].gained == [0] * M and full[0].seconds_used == 0.0
    free = halda_solve_bounded(devs, model, k_candidates=[k], kv_bits="4bit", route="tables")
    assert full[-1].obj_value == free.obj_value and full[-1].regret == 0.0
    assert all(p.regret == p.obj_value - free.obj_value >= 0.0 for p in full)
    for p in full:
        assert p.gained == [max(0, a - b) for a, b in zip(p.plan.w, w0)]
        assert all(g <= c for g, c in zip(p.gained, p.caps))
        assert p.seconds_used == max(g / x for g, x in zip(p.gained, sd)) * group and p.seconds_used <= p.seconds
    assert any(p.obj_value < full[0].obj_value for p in full[1:-1])  # an interior point improves on "w pinned"
    # a cut in seconds (between two points: seconds / (k b_layer) need not round back onto a breakpoint) keeps
    # the points below it
    cut = halda_reload_frontier(devs, model, inc, max_seconds=0.5 * (full[5].seconds + full[6].seconds),
                                max_points=4096, kv_bits="4bit")
    assert [p.seconds for p in cut] == [p.seconds for p in full[:6]]
    assert [result_key(p.plan) for p in cut] == [result_key(p.plan) for p in full[:6]]


# ------------------------------------------------------------------ 7. the CLI
def test_cli_prints_the_reload_frontier(tmp_path):
    from distilp_amd.cli import solver as cli

    profile = str(REPO / "test" / "profiles" / "llama_3_70b" / "online")
    sol = tmp_path / "sol.json"
    base = ["--profile", profile, "--quiet", "--no-plot"]

    def run(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert cli.main(base + extra) == 0
        return buf.getvalue().splitlines()

    run(["--save-solution", str(sol)])
    plain = run(["--evaluate-solution", str(sol)])
    lines = run(["--evaluate-solution", str(sol), "--reload-frontier"])
    assert lines[:len(plain)] == plain
    extra = lines[len(plain):]
    devices, model = cli.load_from_profile_folder(profile)
    inc = cli.load_incumbent(str(sol), devices)
    assert extra == cli.reload_lines(devices, model, inc, None) and len(extra) >= 1
    pat = re.compile(r"reload (\d+): seconds=\d+\.\d{6}, obj=-?\d+\.\d{6}, regret=-?\d+\.\d{6}, gained=\[[\d, ]+\]$")
    assert [int(pat.match(ln).group(1)) for ln in extra] == list(range(len(extra)))
    assert extra[0].startswith("reload 0: seconds=0.000000") and extra[0].endswith("gained=[0, 0]")
    # the incumbent is this fleet's optimum: nothing is gained by any reload
    assert all("regret=0.000000" in ln or "regret=-0.000000" in ln for ln in extra)
    two = run(["--evaluate-solution", str(sol), "--reload-frontier", "0"])
    assert two[len(plain):] == extra[:1]
