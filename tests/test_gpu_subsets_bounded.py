"""Exact device selection under boxes on the GPU (libhalda halda_solve_subsets_boxed). (A) Bit for bit: every
frontier point equals the strict earliest arg-min, in NumPy, over what halda_solve_subfleets_boxed_host writes on
its expansion path for every (candidate list, box) -- on the register, table and expansion routes, on path 1, and
with a launch cut inside a (box, fleet, d) group. (B) The exact oracle per (list, gathered bounds), where the
boxes bind. The route is asserted in every case."""

import contextlib
import ctypes
import io
import json
import math

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_select_devices_exact, halda_solve_bounded_batch, halda_subset_frontier
from distilp_amd.solver import subfleets_bounded as sb
from distilp_amd.solver import subsets_bounded as sx
from distilp_amd.solver._abi import (HaldaBoxesC, HaldaFleetResultC, HaldaSubBoxesC, HaldaSubfleetsC,
                                     HaldaSubsetFrontierC, HaldaSubsetsC)
from distilp_amd.solver.fleets import _host_struct, fleet_table, model_struct
from distilp_amd.solver.subfleets import pack_items

from . import bounds_cases as bc
from . import box_cases as xc
from . import deep_cases as dc
from . import subsets_cases as sc
from . import tied_cases as tc
from .test_gpu_boxes import FILL, IMAX, planes_of

pytestmark = pytest.mark.gpu

FIELDS = ("status", "obj", "mask", "best_k")


@pytest.fixture
def ctx():
    c = lh.get_context(0)
    yield c
    sx.set_subsets_boxed_path(c, 0)
    sx.set_subsets_boxed_chunk(c, 0)
    sb.set_subfleets_boxed_path(c, 0)


def mask_of(devs):
    return sum(1 << i for i in devs)


def frontier(ctx, table, model, ks, D, planes, keeps=None, nb=None, want_rc=0, boxed=True):
    """One halda_solve_subsets_boxed_host call (boxed=False: halda_solve_subsets_host): the four arrays
    [n_box, n_fleets, D + 1], pre-filled with -7, and the route."""
    keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in planes]
    nb = next((len(a) for a in keep if a is not None), 1) if nb is None else nb
    shape = (max(nb, 1) if nb <= 65535 else 1, table.n_fleets, D + 1)
    o = {"status": np.full(shape, -7, np.int32), "obj": np.full(shape, -7.0), "mask": np.full(shape, 7, np.uint64),
         "best_k": np.full(shape, -7, np.int32)}
    fs, hold = _host_struct(table)
    km = None if keeps is None else np.asarray([mask_of(k) for k in keeps], np.uint64)
    sub, fr = HaldaSubsetsC(D, lh.ptr(km)), HaldaSubsetFrontierC(*[lh.ptr(o[f]) for f in FIELDS])
    m, karr = model_struct(model, bc.KV), np.asarray(ks, np.int32)
    if boxed:
        bx = HaldaBoxesC(nb, *[lh.ptr(a) for a in keep])
        rc = ctx.lib.halda_solve_subsets_boxed_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
                                                    karr.ctypes.data, len(ks), ctypes.byref(bx), ctypes.byref(fr))
    else:
        rc = ctx.lib.halda_solve_subsets_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
                                              karr.ctypes.data, len(ks), ctypes.byref(fr))
    assert rc == want_rc, lh.last_error(ctx.lib)
    return o, (sx.last_subsets_boxed_route(ctx) if boxed else None)


def brute_force(ctx, table, model, ks, D, planes, keeps=None):
    """Reference (A): every candidate list under every box through halda_solve_subfleets_boxed_host on its expansion
    path, then the strict earliest arg-min per (box, fleet, d) in NumPy. Also, per point, how many candidates share
    the minimum."""
    sizes, nb = table.sizes().tolist(), len(planes[0])
    keeps = keeps or [()] * len(sizes)
    items, box, groups = [], [], {}
    for b in range(nb):
        for f, M in enumerate(sizes):
            for d in range(sc.limit_of(M, keeps[f], D) + 1):
                cands = sc.candidates(M, keeps[f], d)
                groups[(b, f, d)] = (len(items), cands)
                items += [(f, list(kept)) for _, kept in cands]
                box += [b] * len(cands)
    parent, sub_off, sub_idx = pack_items(np.asarray(sizes, np.int64), items)
    lens, n = np.diff(sub_off), len(parent)
    best_k, obj = np.zeros(n, np.int32), np.zeros(n)
    w, nn = np.zeros(int(sub_off[-1]), np.int32), np.zeros(int(sub_off[-1]), np.int32)
    res = HaldaFleetResultC(lh.ptr(best_k), lh.ptr(obj), lh.ptr(w), lh.ptr(nn), None, None, None, None, None)
    it = HaldaSubfleetsC(n, int(lens.min()), int(lens.max()), lh.ptr(parent), lh.ptr(sub_off), lh.ptr(sub_idx))
    keep = [np.ascontiguousarray(a, np.int32) for a in planes]
    ib = np.asarray(box, np.int32)
    sbx = HaldaSubBoxesC(nb, *[lh.ptr(a) for a in keep], lh.ptr(ib))
    fs, hold = _host_struct(table)
    m, karr = model_struct(model, bc.KV), np.asarray(ks, np.int32)
    sb.set_subfleets_boxed_path(ctx, 1)
    rc = ctx.lib.halda_solve_subfleets_boxed_host(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                  karr.ctypes.data, len(ks), ctypes.byref(sbx), ctypes.byref(res))
    sb.set_subfleets_boxed_path(ctx, 0)
    assert rc == 0, lh.last_error(ctx.lib)
    shape = (nb, len(sizes), D + 1)
    want = {"status": np.full(shape, lh.STATUS_INFEASIBLE, np.int32), "obj": np.full(shape, math.inf),
            "mask": np.zeros(shape, np.uint64), "best_k": np.zeros(shape, np.int32)}
    tied = np.zeros(shape, np.int64)
    for at, (a, cands) in groups.items():
        o = obj[a:a + len(cands)]
        j = int(np.flatnonzero(o == o.min())[0])  # strict <: the earliest minimum
        if o[j] < math.inf:
            tied[at] = int((o == o[j]).sum())
            want["status"][at], want["obj"][at] = lh.STATUS_OPTIMAL, o[j]
            want["mask"][at], want["best_k"][at] = mask_of(cands[j][0]), best_k[a + j]
    return want, tied


def same(a, b, what=None):
    for f in FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def cap_planes(table, rows):
    """[n_box, nd] planes from per-box (w_max, n_max) scalars (here: the even share + 2, and a GPU share <= 2)."""
    nd = table.n_devices
    return [np.full((len(rows), nd), FILL[0], np.int32), np.asarray([[r[0]] * nd for r in rows], np.int32),
            np.full((len(rows), nd), FILL[2], np.int32), np.asarray([[r[1]] * nd for r in rows], np.int32)]


# name -> (route, fleets, model, ks, max_drop, keeps, planes); built once
_SHAPES = {}


def shape(model, name):
    if name in _SHAPES:
        return _SHAPES[name]
    if name == "reg-odd":  # 211 candidates x 3 fleets x 2 boxes: not a multiple of the four waves per workgroup
        par = [(20, s) for s in range(3)]
        s = ("register", par, model, [1], 2, None, planes_of(model, par, 1, ("box1", "nmax")))
    elif name == "reg-64":  # lane 63, the M == 64 mask and the last combo bit; device 0 kept
        s = ("register", [(64, 0)], model, [1], 1, [(0,)], planes_of(model, [(64, 0)], 1, ("box1", "nmax")))
    elif name == "tab":  # every subset of the 4- and 8-device fleets; the one-device fleet has the point d = 0 alone
        par = [(4, 0), (8, 1), (16, 2), (1, 3)]
        s = ("tables", par, model, [1, 2, 4, 5], 7, None, planes_of(model, par, 2, ("box1", "nmax")))
    elif name == "exp":  # 64 x (512 - 63 + 1) table entries: a slice beyond the LDS budget; two droppable devices
        keep = tuple(i for i in range(64) if i not in (1, 2))
        s = ("expand", [(64, 0)], dc.model_at(model, 512), [1], 1, [keep], None)
    elif name == "tie":  # a duplicated 16-device fleet: equal candidates, the earliest must win
        case = tc.cases("T16p")[0]
        s = ("tables", tc.devices(case), tc.model_of(case), [1, 2, 4, 5], 2, None, None)
    route, par, mdl, ks, D, keeps, planes = s
    fleets = [par] if name == "tie" else [list(bc.devices(M, sd)) for M, sd in par]
    table = fleet_table(fleets, mdl)
    if planes is None:
        planes = cap_planes(table, [(int(mdl.L) // ks[0] // table.n_devices + 2, IMAX), (IMAX, 2)])
    _SHAPES[name] = (route, table, mdl, ks, D, keeps, planes)
    return _SHAPES[name]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", ["reg-odd", "reg-64", "tab", "exp", "tie"])
def test_frontier_equals_the_arg_min_over_every_boxed_candidate(ctx, llama_online_model, name, path):
    route, table, model, ks, D, keeps, planes = shape(llama_online_model, name)
    sx.set_subsets_boxed_path(ctx, path)
    got, r = frontier(ctx, table, model, ks, D, planes, keeps)
    assert r == ("expand" if path == 1 else route), name
    want, tied = brute_force(ctx, table, model, ks, D, planes, keeps)
    same(got, want, name)
    assert (want["status"] == lh.STATUS_OPTIMAL).any() and (want["mask"][:, :, 1:] != 0).any()
    if name == "tab":  # the one-device fleet past d = 0, and the 4-device fleet past d = 3: no candidate
        assert (got["status"][:, 3, 1:] == lh.STATUS_INFEASIBLE).all() and (got["obj"][:, 0, 4:] == math.inf).all()
    if name == "tie":  # candidates of equal value exist, and the winner is the first of them (strict arg-min above)
        assert (tied > 1).any()
    # the boxes matter: some point differs from the unbounded frontier
    free, _ = frontier(ctx, table, model, ks, D, [None] * 4, keeps, boxed=False)
    assert any(got[f][b].tobytes() != free[f][0].tobytes() for f in FIELDS for b in range(len(planes[0])))


@pytest.mark.parametrize("path", [0, 1])
def test_a_launch_cut_inside_a_group_folds_to_the_same_bits(ctx, llama_online_model, path):
    """190 candidates per (box, fleet) at d = 2: launches of 77 items cut every group, most of them twice."""
    route, table, model, ks, D, keeps, planes = shape(llama_online_model, "reg-odd")
    sx.set_subsets_boxed_path(ctx, path)
    whole, r = frontier(ctx, table, model, ks, D, planes, keeps)
    sx.set_subsets_boxed_chunk(ctx, 77)
    cut, r2 = frontier(ctx, table, model, ks, D, planes, keeps)
    assert r == r2 == ("expand" if path else route)
    same(cut, whole)


def test_bounds_follow_the_parent_index_and_vanish_with_the_device(ctx, llama_online_model):
    """w_max_j < w_min_j on droppable device j = 5: nothing is feasible while j is kept, so d = 0 is INFEASIBLE and
    the d = 1 winner drops exactly j; the devices behind j keep their own (free) entries."""
    model, j = llama_online_model, 5
    table = fleet_table([list(bc.devices(8, s)) for s in range(2)], model)
    planes = [np.full((1, 16), FILL[a], np.int32) for a in range(4)]
    planes[0][0, [j, 8 + j]], planes[1][0, [j, 8 + j]] = 5, 4
    for ks, route in (([1], "tables"), ([2, 4], "tables")):
        got, r = frontier(ctx, table, model, ks, 1, planes)
        assert r == route
        assert (got["status"][0, :, 0] == lh.STATUS_INFEASIBLE).all() and (got["obj"][0, :, 0] == math.inf).all()
        assert (got["status"][0, :, 1] == lh.STATUS_OPTIMAL).all() and got["mask"][0, :, 1].tolist() == [1 << j] * 2
        same(got, brute_force(ctx, table, model, ks, 1, planes)[0])


@pytest.mark.parametrize("name", ["reg-odd", "tab"])
def test_without_bounds_the_frontier_is_the_unbounded_call(ctx, llama_online_model, name):
    route, table, model, ks, D, keeps, _ = shape(llama_online_model, name)
    got, r = frontier(ctx, table, model, ks, D, [None] * 4, keeps, nb=1)
    assert r == route
    free, _ = frontier(ctx, table, model, ks, D, [None] * 4, keeps, boxed=False)
    same(got, free, name)


def test_argument_errors_launch_nothing(ctx, llama_online_model):
    _, table, model, ks, D, keeps, planes = shape(llama_online_model, "tab")
    for kw, text in (({"nb": 0}, "n_box"), ({"nb": 65536}, "n_box"), ({"D": 16}, "max_drop"), ({"D": 64}, "max_drop"),
                     ({"keeps": [(4,), (), (), ()]}, "keep_mask"), ({"ks": [2, 1]}, "ascending")):
        a = {"ks": ks, "D": D, "keeps": keeps, "nb": None, **kw}
        o, _ = frontier(ctx, table, model, a["ks"], a["D"], planes, a["keeps"], a["nb"], want_rc=-22)
        assert text in lh.last_error(ctx.lib), kw
        assert all((o[f] == (7 if f == "mask" else -7)).all() for f in FIELDS)  # nothing was written
    for setter, bad in ((sx.set_subsets_boxed_path, 2), (sx.set_subsets_boxed_chunk, (1 << 22) + 1)):
        with pytest.raises(RuntimeError):
            setter(ctx, bad)


# ------------------------------------------------------------------ (B) the exact oracle
ORACLE_KINDS = ("box1", "off", "half", "pin")
ORACLE_CASES = [(8, 1, 1, 2), (8, 1, 2, 2), (5, 0, 1, 4)]  # (M, seed, k, max_drop)


def oracle_frontier(model, M, seed, k, D):
    """(planes, bounded, free): per (box, d) the (objective or inf, dropped tuple or None, unique, feasible
    candidates, runner-up objective) of the exact oracle over every (kept list, gathered bounds), the strict earliest
    minimum; `free` is the same without bounds. GPU-free."""
    devs, W = list(bc.devices(M, seed)), int(model.L) // k
    planes = planes_of(model, [(M, seed)], k, ORACLE_KINDS)
    free = (np.ones((1, M), np.int64), np.full((1, M), W), np.zeros((1, M), np.int64), np.full((1, M), IMAX))
    rows = []
    for pl in (planes, free):
        out = {}
        for b, d in ((b, d) for b in range(len(pl[0])) for d in range(D + 1)):
            ok = []
            for gone, kept in sc.candidates(M, (), d):
                box = [p[b, list(kept)].tolist() for p in pl]
                box[0], box[1] = [max(1, v) for v in box[0]], [min(W, v) for v in box[1]]
                st, _, _, obj, unique = xc.exact_answer(model, [devs[i] for i in kept], k, box)
                if st == 0:
                    ok.append((obj, gone, unique))
            j = min(range(len(ok)), key=lambda i: ok[i][0], default=None)  # min: the first among equals
            runner = min((v[0] for i, v in enumerate(ok) if i != j), default=math.inf)
            out[(b, d)] = (math.inf, None, True, 0, runner) if j is None else ok[j] + (len(ok), runner)
        rows.append(out)
    return planes, rows[0], rows[1]


@pytest.mark.parametrize("M,seed,k,D", ORACLE_CASES)
def test_frontier_equals_the_exact_oracle(ctx, llama_online_model, M, seed, k, D):
    planes, bounded, free = oracle_frontier(llama_online_model, M, seed, k, D)
    # the boxes bind: by the oracle alone, enough feasible candidates and a bounded point whose winner or objective
    # differs from the unbounded frontier's
    differ = [at for at, v in bounded.items() if v[1] != free[(0, at[1])][1]
              or (v[1] is not None and bc.rel(v[0], free[(0, at[1])][0]) > 1e-6)]
    assert sum(v[3] for v in bounded.values()) >= M and differ
    table = fleet_table([list(bc.devices(M, seed))], llama_online_model)
    got, r = frontier(ctx, table, llama_online_model, [k], D, planes)
    assert r == "tables"
    for (b, d), (obj, gone, unique, _, runner) in bounded.items():
        case = (M, seed, k, b, d)
        if gone is None:
            assert got["status"][b, 0, d] == lh.STATUS_INFEASIBLE and got["mask"][b, 0, d] == 0, case
            continue
        assert got["status"][b, 0, d] == lh.STATUS_OPTIMAL and got["best_k"][b, 0, d] == k, case
        assert bc.rel(float(got["obj"][b, 0, d]), obj) <= 1e-9, case
        if unique and not sc.near_tie(obj, runner):
            assert int(got["mask"][b, 0, d]) == mask_of(gone), case


# ------------------------------------------------------------------ Python and CLI
def key(r):
    return None if r is None else (r.k, list(r.w), list(r.n), r.obj_value, r.sets)


def by_lists(devs, model, box, D, keep, ks):
    """The frontier by halda_solve_bounded_batch over every materialised list, the strict earliest minimum."""
    pts = []
    for d in range(D + 1):
        best = None
        for gone, kept in sc.candidates(len(devs), keep, d):
            r = halda_solve_bounded_batch([[devs[i] for i in kept]], model, [sx.gather_bounds(box, kept)], ks,
                                          kv_bits="4bit", route="tables")[0]
            if r is not None and (best is None or r.obj_value < best[1].obj_value):
                best = (list(gone), r)
        pts.append(best)
    return pts


def test_python_entries_equal_the_bounded_batch_over_materialised_lists(llama_online_model):
    model, devs, ks = llama_online_model, list(bc.devices(8, 3)), [1, 2, 4]
    box = (None, [30, 30, 20, 20, 20, 20, 30, 30], None, [IMAX, 0, IMAX, 5, IMAX, IMAX, 0, IMAX])
    pts = halda_subset_frontier(devs, model, 2, [0], ks, kv_bits="4bit", bounds=box)
    want = by_lists(devs, model, box, 2, (0,), ks)
    assert len(pts) == 3 and any(w is not None for w in want)
    for p, w in zip(pts, want):
        assert (p.result is None) == (w is None)
        if w is not None:
            assert p.dropped == w[0] and key(p.result) == key(w[1]) and 0 in p.kept
    kept, r = halda_select_devices_exact(devs, model, 2, [0], ks, kv_bits="4bit", bounds=box)
    best = min((w for w in want if w is not None), key=lambda w: w[1].obj_value)  # min: the first among equals
    assert kept == [i for i in range(8) if i not in best[0]] and key(r) == key(best[1])
    rows = sx.halda_subset_frontier_boxes(devs, model, [box, None], 2, [0], ks, kv_bits="4bit")
    assert [key(p.result) for p in rows[0]] == [key(p.result) for p in pts]
    free = halda_subset_frontier(devs, model, 2, [0], ks, kv_bits="4bit")
    assert [(p.dropped, p.obj_value) for p in rows[1]] == [(p.dropped, p.obj_value) for p in free]


def test_cli_select_devices_bounded_on_an_eight_device_folder(tmp_path):
    """--cpu-only on two devices, two others kept (one by name), D = 2; then the --max-move form (a move box around a
    saved plan, at that plan's k). Both against the brute force over materialised lists."""
    from distilp_amd.cli.solver import bounded_box, cpu_only_n_max, load_from_profile_folder, load_incumbent, main
    from distilp_amd.synth import load_model_dict

    for i, dev in enumerate(bc.devices(8, 3)):
        (tmp_path / f"dev{i}.json").write_text(dev.model_dump_json())
    (tmp_path / "model_profile.json").write_text(json.dumps(load_model_dict()))
    devs, model = load_from_profile_folder(str(tmp_path))
    base, saved = ["--profile", str(tmp_path), "--no-plot", "--quiet"], str(tmp_path / "plan.out")

    def run(args):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert main(base + args) == 0
        return out.getvalue()

    def lines_of(box, D, keep, ks):
        want = by_lists(devs, model, box, D, keep, ks)
        best = min((w for w in want if w is not None), key=lambda w: w[1].obj_value)  # min: the first among equals
        names = ", ".join(devs[i].name for i in range(8) if i not in best[0])
        return [f"drop {d} (bounded): infeasible" if w is None else
                f"drop {d} (bounded): dropped=[{', '.join(devs[i].name for i in w[0])}], k={w[1].k}, "
                f"obj={w[1].obj_value:.6f}" for d, w in enumerate(want)] + [f"selected (bounded): kept=[{names}]"]

    cpu = ["--cpu-only", "0", "4"]
    plain = run(cpu + ["--save-solution", saved])
    both = run(cpu + ["--save-solution", saved, "--select-devices-bounded", "2", "--keep", "2", devs[3].name])
    assert both.startswith(plain)  # the usual output, unchanged
    want = lines_of((None, None, None, cpu_only_n_max(devs, ["0", "4"])), 2, (2, 3), None)
    assert both[len(plain):].splitlines() == want and any("dropped=[" in ln for ln in want[1:3])
    plan = load_incumbent(saved, devs)
    move = ["--evaluate-solution", saved, "--max-move", "6"]
    got = run(move + ["--select-devices-bounded", "1", "--keep", "7"])[len(run(move)):].splitlines()
    want = lines_of(bounded_box(None, plan, 6, None), 1, (7,), [plan[0]])
    assert got == want and any("dropped=[" in ln for ln in want[1:2])
