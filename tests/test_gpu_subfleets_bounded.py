"""Sub-fleets under boxes on the GPU (libhalda halda_solve_subfleets_boxed): every output equals, bit for bit, the
halda_solve_fleets_boxed_host call on the materialised lists with gathered bounds under bounds path 3, on the
register route (halda_sweep_subfleets_box_kernel), the table route (halda_sweep_subfleets_box_tables_kernel) and
the expansion route; the expansion test path gives the fused routes' bits; a NULL array is its "no bound" fill;
without bounds the outputs are halda_solve_subfleets'; the items equal the exact oracle; and the Python and CLI
entries built on the call. The route is asserted in every case.

test_items_equal_the_exact_oracle's parents of 4 and 16 devices reach the table route only (a list of 15 devices
has L - M' + 1 = 66 > 64 states at k = 1), so the register route's oracle case is a parent of 24 devices."""

import contextlib
import ctypes
import io

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import halda_leave_one_out, halda_solve_bounded_batch, halda_solve_subfleets_bounded
from distilp_amd.solver import subfleets_bounded as sb
from distilp_amd.solver._abi import HaldaSubBoxesC, HaldaSubfleetsC
from distilp_amd.solver.fleets import _host_struct, fleet_table
from distilp_amd.solver.subfleets import gather_table, leave_one_out_items, pack_items

from . import bounds_cases as bc
from . import box_cases as xc
from .conftest import REPO
from .test_gpu_boxes import FILL, Host, planes_of, same

pytestmark = pytest.mark.gpu

IMAX = 2**31 - 1


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    bd.set_bounds_path(c, 0)
    sb.set_subfleets_boxed_path(c, 0)


class Run:
    """Parents [(M, seed)] packed once, items as index arrays, and the materialised lists as test_gpu_boxes.Host:
    its guarded output arrays and compact x_off are the items' (fleet i of the gathered table is item i)."""

    def __init__(self, model, parents, arrays, ks, item_box=None):
        self.table = fleet_table([list(bc.devices(M, s)) for M, s in parents], model)
        self.parent, self.sub_off, self.sub_idx = arrays
        self.lens = np.diff(self.sub_off)
        n = len(self.parent)
        self.item_box = np.asarray(np.arange(n) % 2 if item_box is None else item_box, np.int32)
        self.ref = Host(gather_table(self.table, *arrays), model, ks)
        self.fs, self.keep = _host_struct(self.table)
        self.g = np.repeat(self.table.dev_off[self.parent.astype(np.int64)], self.lens) + self.sub_idx

    def items(self):
        return HaldaSubfleetsC(len(self.parent), int(self.lens.min()), int(self.lens.max()), lh.ptr(self.parent),
                               lh.ptr(self.sub_off), lh.ptr(self.sub_idx))

    def solve(self, ctx, planes, item_box="own", nb=None, want_rc=0):
        """One halda_solve_subfleets_boxed_host call; planes: four [n_box, nd] int arrays or None each."""
        keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in planes]
        ib = self.item_box if isinstance(item_box, str) else item_box
        nb = next((len(a) for a in keep if a is not None), 1) if nb is None else nb
        o, res, _ = self.ref.outputs(1)
        it, r = self.items(), self.ref
        b = HaldaSubBoxesC(nb, *[lh.ptr(a) for a in keep], lh.ptr(ib))
        rc = ctx.lib.halda_solve_subfleets_boxed_host(ctx.ctx, ctypes.byref(r.m), ctypes.byref(self.fs), ctypes.byref(it),
                                                      r.ks.ctypes.data, r.nk, ctypes.byref(b), ctypes.byref(res))
        assert rc == want_rc, lh.last_error(ctx.lib)
        return o if want_rc else (Host.collect(o, 1), sb.last_subfleets_boxed_route(ctx))

    def gathered(self, planes):
        """The listed devices' entries of their items' boxes, in the materialised table's layout."""
        b = np.repeat(self.item_box, self.lens)
        return [None if p is None else p[b, self.g] for p in planes]

    def unbounded(self, ctx):
        o, res, _ = self.ref.outputs(1)
        it, r = self.items(), self.ref
        rc = ctx.lib.halda_solve_subfleets_host(ctx.ctx, ctypes.byref(r.m), ctypes.byref(self.fs), ctypes.byref(it),
                                                r.ks.ctypes.data, r.nk, ctypes.byref(res))
        assert rc == 0, lh.last_error(ctx.lib)
        return Host.collect(o, 1)


def lists(sizes, items):
    return pack_items(np.asarray(sizes, np.int64), items)


# name -> (route, the single call's route, parents [(M, seed)], item arrays, ks, the k the boxes are built at)
SHAPES = {
    # 75 items of 24 devices: not a multiple of the four waves per workgroup
    "reg": ("register", "fused", [(25, s) for s in range(3)], leave_one_out_items([25] * 3), [1], 1),
    # lists of 1, 3, 7, 15: one descending, one with a repeat, one whose head is not the parent's device 0
    "tab": ("tables", "tables", [(4, 0), (8, 1), (16, 2)],
            lists([4, 8, 16], [(0, [2]), (0, [3, 1, 0]), (1, list(range(1, 8))), (1, [6, 5, 4, 3, 2, 1, 0]),
                               (2, list(range(15))), (2, [5, 5] + list(range(3, 16))), (1, [7])]), [1, 2, 4, 5], 2),
    "exp": ("expand", "general", [(72, 0)], lists([72], [(0, list(range(1, 71)))]), [1, 2], 1),
}
_RUNS = {}


def shape_run(model, name):
    """(Run, planes) of a shape, built once: box 0 a move box (box_cases "box1"), box 1 an n_max-only cap."""
    if name not in _RUNS:
        _, _, parents, arrays, ks, k = SHAPES[name]
        _RUNS[name] = (Run(model, parents, arrays, ks), planes_of(model, parents, k, ("box1", "nmax")))
    return _RUNS[name]


# ------------------------------------------------------------------ 1. bits per route
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_items_equal_the_boxed_call_on_the_materialised_lists(ctx, llama_online_model, name):
    route, single = SHAPES[name][:2]
    run, planes = shape_run(llama_online_model, name)
    assert set(run.item_box.tolist()) == {0, 1} or name == "exp"
    got, r = run.solve(ctx, planes)
    assert r == route, name
    want, rb = run.ref.boxed(ctx, run.gathered(planes))
    assert rb == single, name
    same(got, want, name)
    assert (want["best_k"] > 0).any()  # the comparison is not of zeros
    if name != "exp":  # path 1: always expansion, the fused routes' bits; the context's bounds path comes back
        bd.set_bounds_path(ctx, 1)
        sb.set_subfleets_boxed_path(ctx, 1)
        exp, r = run.solve(ctx, planes)
        assert r == "expand" and bd.last_bounds_route(ctx) == single and ctx.paths["bounds"] == 1
        same(exp, got, name)


@pytest.mark.parametrize("name", ["reg", "tab"])
def test_a_null_array_is_its_no_bound_fill(ctx, llama_online_model, name):
    run, planes = shape_run(llama_online_model, name)
    for a in range(4):
        got, r = run.solve(ctx, [None if i == a else p for i, p in enumerate(planes)])
        want, r2 = run.solve(ctx, [np.full_like(p, FILL[a]) if i == a else p for i, p in enumerate(planes)])
        assert r == r2 == SHAPES[name][0]
        same(got, want, (name, a))
    # a NULL item_box is box 0 for every item
    got, _ = run.solve(ctx, planes, item_box=None)
    want, _ = run.solve(ctx, planes, item_box=np.zeros_like(run.item_box))
    same(got, want, name)


# ------------------------------------------------------------------ 3. identity: no bounds, halda_solve_subfleets
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_without_bounds_the_outputs_are_the_unbounded_call(ctx, llama_online_model, name):
    run, _ = shape_run(llama_online_model, name)
    got, r = run.solve(ctx, [None] * 4, item_box=None)
    assert r == SHAPES[name][0]
    same(got, run.unbounded(ctx), name)


def test_argument_errors_launch_nothing(ctx, llama_online_model):
    run, planes = shape_run(llama_online_model, "tab")
    bad_box = run.item_box.copy()
    bad_box[3] = 2
    for kw, text in (({"nb": 0}, "n_box"), ({"nb": 65536}, "n_box"), ({"item_box": bad_box}, "item 3 has box 2")):
        o = run.solve(ctx, planes, want_rc=-22, **kw)
        assert text in lh.last_error(ctx.lib)
        assert all((a == -7).all() for a in o.values())  # nothing was written
    with pytest.raises(RuntimeError):
        sb.set_subfleets_boxed_path(ctx, 2)


# ------------------------------------------------------------------ 2. the exact oracle
ORACLE_KINDS = ("box1", "off", "half", "pin", "cross")


@pytest.mark.parametrize("M,k,route", [(4, 1, "tables"), (4, 2, "tables"), (16, 1, "tables"), (16, 2, "tables"),
                                       (24, 1, "register")])
def test_items_equal_the_exact_oracle(ctx, llama_online_model, M, k, route):
    """Parent devices(M, 0), every device dropped in turn under each kind's box restricted to the survivors."""
    model, W = llama_online_model, int(llama_online_model.L) // k
    arrays = leave_one_out_items([M] * len(ORACLE_KINDS))
    arrays = (np.zeros_like(arrays[0]), arrays[1], arrays[2])  # every item of the one parent; kind b's items use box b
    run = Run(model, [(M, 0)], arrays, [k], item_box=np.repeat(np.arange(len(ORACLE_KINDS)), M))
    planes = planes_of(model, [(M, 0)], k, ORACLE_KINDS)
    got, r = run.solve(ctx, planes)
    assert r == route
    devs = list(bc.devices(M, 0))
    free = ([1] * (M - 1), [W] * (M - 1), [0] * (M - 1), [IMAX] * (M - 1))
    feasible = binding = 0
    for b, kind in enumerate(ORACLE_KINDS):
        for i in range(M):
            it, a = b * M + i, (b * M + i) * (M - 1)
            keep = [j for j in range(M) if j != i]
            sub = [devs[j] for j in keep]
            box = [p[b, keep].tolist() for p in planes]
            box[0], box[1] = [max(1, v) for v in box[0]], [min(W, v) for v in box[1]]
            st, x, _, obj, unique = xc.exact_answer(model, sub, k, box)
            case = (M, k, kind, i)
            if st != 0:
                assert got["status"][0, it] == lh.STATUS_INFEASIBLE and got["best_k"][0, it] == 0, case
                continue
            feasible += 1
            assert got["status"][0, it] == lh.STATUS_OPTIMAL and got["best_k"][0, it] == k, case
            assert bc.rel(float(got["obj_value"][0, it:it + 1].view(np.float64)[0]), obj) <= 1e-9, case
            if unique:
                assert got["w"][0, a:a + M - 1].tolist() == [int(round(v)) for v in x[:M - 1]], case
                assert got["n"][0, a:a + M - 1].tolist() == [int(round(v)) for v in x[M - 1:2 * M - 2]], case
            st0, _, _, obj0, _ = xc.exact_answer(model, sub, k, free)
            binding += int(st0 == 0 and bc.rel(obj, obj0) > 1e-6)
    assert feasible >= M and binding >= 1  # the bounds bind: the oracle alone shows a bounded optimum that differs


# ------------------------------------------------------------------ 4. Python and CLI
def key(r):
    return None if r is None else (r.k, list(r.w), list(r.n), r.obj_value, r.sets)


def test_leave_one_out_with_bounds_equals_the_bounded_batch(llama_online_model):
    model, devs = llama_online_model, list(bc.devices(6, 3))
    n_max = [IMAX, 0, IMAX, 5, IMAX, IMAX]
    for box in ((None, [30, 30, 20, 20, 20, 20], None, n_max), ([2] * 6, [25] * 6)):
        got = halda_leave_one_out(devs, model, [1, 2, 4], kv_bits="4bit", bounds=box)
        for i in range(6):
            keep = [j for j in range(6) if j != i]
            sub = tuple(None if a is None else [a[j] for j in keep] for a in box)
            want = halda_solve_bounded_batch([[devs[j] for j in keep]], model, [sub], [1, 2, 4], kv_bits="4bit",
                                             route="tables")[0]
            assert key(got[i]) == key(want), i
        items = [(0, [j for j in range(6) if j != i], 0) for i in range(6)]
        assert [key(r) for r in halda_solve_subfleets_bounded([devs], model, items, [[box]], [1, 2, 4], "4bit")] == \
               [key(r) for r in got]
    assert any(r is not None for r in got)
    free = halda_leave_one_out(devs, model, [1, 2, 4], kv_bits="4bit")
    assert [key(r) for r in halda_leave_one_out(devs, model, [1, 2, 4], kv_bits="4bit", bounds=None)] == \
           [key(r) for r in free]


def test_cli_leave_one_out_bounded_lines(monkeypatch, fixtures_golden):
    from distilp_amd.cli.solver import cpu_only_n_max, load_from_profile_folder, main

    monkeypatch.chdir(REPO)
    argv = fixtures_golden["cli"]["online_default"]["argv"]
    plain, both = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(plain):
        assert main(argv + ["--cpu-only", "0"]) == 0
    with contextlib.redirect_stdout(both):
        assert main(argv + ["--cpu-only", "0", "--leave-one-out-bounded"]) == 0
    assert both.getvalue().startswith(plain.getvalue())  # the usual output, unchanged
    devs, model = load_from_profile_folder("llama_3_70b/online")
    res = halda_leave_one_out(devs, model, kv_bits="4bit", bounds=(None, None, None, cpu_only_n_max(devs, ["0"])))
    want = [f"without {d.name} (bounded): " + ("infeasible" if r is None else f"k={r.k}, obj={r.obj_value:.6f}")
            for d, r in zip(devs, res)]
    assert both.getvalue()[len(plain.getvalue()):].splitlines() == want and len(want) == 2
