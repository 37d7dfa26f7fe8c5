"""One table under many boxes and the reload-time frontier, without a GPU: reload_caps on hand-written numbers
(the counting rule, shared points, the cuts), the argument checks of the boxes entries (raised before any packing
or library call), the planes' layout, the C surface (include/halda_boxes.h against the binding) and the CLI lines. The seeds test_gpu_boxes.py uses for the
reload frontier are shown here, with the exact oracle, to improve strictly at an interior point."""

import ctypes
import math
import re
import shutil
import subprocess

import numpy as np
import pytest

from distilp_amd.cli import solver as cli
from distilp_amd.solver import _abi
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import boxes as bx
from distilp_amd.solver._abi import HaldaBoxesC
from distilp_amd.solver.coefficients import HALDAResult
from distilp_amd.solver.fleets import fleet_table

from . import bounds_cases as bc
from . import box_cases as xc
from . import budget_cases as gc
from .conftest import REPO

IMAX = 2**31 - 1
# (M, k, seed): the reload-frontier cases of test_gpu_boxes.py
RELOAD_CASES = [(M, k, s) for M in (4, 16) for k in (1, 2) for s in (0, 1)]


# ------------------------------------------------------------------ reload_caps
def test_reload_caps_counts_quotients():
    # W = 8, M = 2: device 0 holds 2 and may gain 5, device 1 holds 3 and may gain 4
    t, caps = bx.reload_caps([2, 3], [4.0, 2.0], 8)
    assert t.dtype == np.float64 and caps.dtype == np.int64
    # 1/4, 2/4 = 1/2, 3/4, 4/4 = 2/2, 5/4, 3/2, 4/2: equal quotients on the two devices are one point
    assert t.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0]
    assert caps.tolist() == [[0, 0], [1, 0], [2, 1], [3, 1], [4, 2], [5, 2], [5, 3], [5, 4]]
    assert (np.diff(caps, axis=0) >= 0).all() and (caps[0] == 0).all()


def test_reload_caps_equal_disks_share_their_points():
    t, caps = bx.reload_caps([1, 1, 1], [5.0, 5.0, 1.0], 6)  # each may gain 6 - 2 - 1 = 3
    assert t.tolist() == [0.0, 0.2, 0.4, 3 / 5.0, 1.0, 2.0, 3.0]
    assert caps[:, 0].tolist() == caps[:, 1].tolist() == [0, 1, 2, 3, 3, 3, 3]
    assert caps[:, 2].tolist() == [0, 0, 0, 0, 1, 2, 3]


def test_reload_caps_full_device_has_no_candidates():
    # device 1 already holds W - (M - 1) = 7 layers: no m for it, its cap stays 0
    t, caps = bx.reload_caps([1, 7, 2], [1.0, 1e9, 2.0], 9)
    assert (caps[:, 1] == 0).all()
    assert caps[-1].tolist() == [9 - 2 - 1, 0, 9 - 2 - 2]
    t1, caps1 = bx.reload_caps([8], [3.0], 8)  # a one-device fleet holds everything
    assert t1.tolist() == [0.0] and caps1.tolist() == [[0]]


def test_reload_caps_cuts():
    full_t, full_caps = bx.reload_caps([2, 3], [4.0, 2.0], 8)
    t, caps = bx.reload_caps([2, 3], [4.0, 2.0], 8, max_points=3)
    assert t.tolist() == full_t[:3].tolist() and caps.tolist() == full_caps[:3].tolist()
    t, caps = bx.reload_caps([2, 3], [4.0, 2.0], 8, max_points=1)
    assert t.tolist() == [0.0] and caps.tolist() == [[0, 0]]
    t, caps = bx.reload_caps([2, 3], [4.0, 2.0], 8, max_seconds_per_layer=1.0)  # t = 1.0 itself stays
    assert t.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0] and caps[-1].tolist() == [4, 2]
    t, caps = bx.reload_caps([2, 3], [4.0, 2.0], 8, max_seconds_per_layer=0.99)
    assert t.tolist() == [0.0, 0.25, 0.5, 0.75]
    t, caps = bx.reload_caps([2, 3], [4.0, 2.0], 8, max_points=4, max_seconds_per_layer=0.0)
    assert t.tolist() == [0.0]
    for bad in ({"max_points": 0}, {"max_points": 2.5}, {"max_seconds_per_layer": -1.0},
                {"max_seconds_per_layer": math.nan}):
        with pytest.raises(ValueError):
            bx.reload_caps([2, 3], [4.0, 2.0], 8, **bad)
    for s in ([4.0], [4.0, 0.0], [4.0, -1.0], [4.0, math.inf]):
        with pytest.raises(ValueError):
            bx.reload_caps([2, 3], s, 8)


def test_reload_caps_never_takes_the_floor_of_a_product():
    """s_disk = 49: t = 1 / 49 and 1 / 49 * 49 < 1 in FP64, so floor(t * s_disk) says 0 layers fit in the time
    one layer takes. The counting rule says 1."""
    s = 49.0
    assert (1.0 / s) * s < 1.0 and math.floor((1.0 / s) * s) == 0
    t, caps = bx.reload_caps([1, 1], [s, 1.0], 4)
    assert t[1] == 1.0 / s and caps[1].tolist() == [1, 0]
    # and at every breakpoint the device that defines it is counted in full
    w0, sd, W = [3, 1, 2, 5], [49.0, 0.1, 3.0, 7.0], 40
    t, caps = bx.reload_caps(w0, sd, W)
    room = [W - 3 - w for w in w0]
    floors = 0
    for j in range(1, len(t)):
        hit = [i for i in range(4) for m in range(1, room[i] + 1) if m / sd[i] == t[j]]
        assert hit, j
        for i in range(4):
            assert caps[j][i] == sum(1 for m in range(1, room[i] + 1) if m / sd[i] <= t[j]), (j, i)
            floors += caps[j][i] != min(room[i], math.floor(t[j] * sd[i]))
    assert floors > 0  # the product's floor does disagree on these numbers
    assert caps[-1].tolist() == room


# ------------------------------------------------------------------ the argument checks, before any library call
@pytest.fixture
def no_library(monkeypatch):
    def absent(*a, **k):
        raise AssertionError("reached the packer or the library")

    monkeypatch.setattr(bx, "get_context", absent)
    monkeypatch.setattr(bx, "fleet_table", absent)


def test_boxes_entries_check_their_arguments_first(no_library, llama_online_model):
    model = llama_online_model
    d4, d3 = list(bc.devices(4, 0)), list(bc.devices(3, 1))
    with pytest.raises(ValueError, match="empty"):
        bx.halda_solve_boxes_batch([d4], model, [])
    with pytest.raises(ValueError, match="empty"):
        bx.halda_solve_boxes(d4, model, [])
    with pytest.raises(ValueError, match="at most 65535"):
        bx.halda_solve_boxes(d4, model, [None] * 65536)
    with pytest.raises(ValueError, match="box 1: 1 bounds for 2 fleets"):
        bx.halda_solve_boxes_batch([d4, d3], model, [[None, None], [None]])
    with pytest.raises(ValueError, match="w_max of 3 entries for a fleet of 4"):
        bx.halda_solve_boxes(d4, model, [None, (None, [1, 2, 3])])
    with pytest.raises(ValueError, match="n_min of 4 entries for a fleet of 3"):
        bx.halda_solve_boxes_batch([d4, d3], model, [[None, (None, None, [0] * 4, None)]])
    with pytest.raises(ValueError, match=">= 1"):
        bx.halda_solve_boxes(d4, model, [([0, 1, 1, 1], None)])
    with pytest.raises(ValueError, match="not an integer"):
        bx.halda_solve_boxes(d4, model, [(None, [1, 2.0, 1, 1])])
    with pytest.raises(ValueError, match="entry of 3 items"):
        bx.halda_solve_boxes(d4, model, [(None, None, None)])
    with pytest.raises(ValueError, match="not a sequence"):
        bx.halda_solve_boxes(d4, model, 5)
    with pytest.raises(ValueError, match="not a sequence"):
        bx.halda_solve_boxes_batch([d4], model, [7])


def test_reload_frontier_checks_its_arguments_first(no_library, llama_online_model):
    model = llama_online_model
    devs, w0 = gc.list_case(model, 4, 1, 0)
    n0 = [0] * 4
    with pytest.raises(ValueError, match="needs an incumbent"):
        bx.halda_reload_frontier(devs, model, None)
    with pytest.raises(ValueError, match="sums to"):
        bx.halda_reload_frontier(devs, model, (2, w0, n0))
    with pytest.raises(ValueError, match="incumbent w of 3 entries"):
        bx.halda_reload_frontier(devs, model, (1, w0[:3], n0))
    with pytest.raises(ValueError, match=">= 1"):
        bx.halda_reload_frontier(devs, model, (1, [0, 1, 1, 78], n0))
    with pytest.raises(ValueError, match="max_points"):
        bx.halda_reload_frontier(devs, model, (1, w0, n0), max_points=0)
    with pytest.raises(ValueError, match="max_points"):
        bx.halda_reload_frontier(devs, model, (1, w0, n0), max_points=65535)
    with pytest.raises(ValueError, match="max_seconds"):
        bx.halda_reload_frontier(devs, model, (1, w0, n0), max_seconds=-1.0)


def test_solve_boxes_table_checks_the_planes(llama_online_model):
    model = llama_online_model
    table = fleet_table([list(bc.devices(4, 0)), list(bc.devices(3, 1))], model)
    ok = np.zeros((2, 7), np.int32)
    for planes in ((None,) * 4, (ok, ok), (ok, np.zeros((3, 7), np.int32), None, None),
                   (np.zeros((2, 6), np.int32), None, None, None), (np.zeros(7, np.int32), None, None, None),
                   (np.zeros((0, 7), np.int32), None, None, None)):
        with pytest.raises(ValueError):
            bx.solve_boxes_table(table, model, [1], planes, 0.5)


def test_box_planes_layout(llama_online_model):
    table = fleet_table([list(bc.devices(4, 0)), list(bc.devices(3, 1))], llama_online_model)
    boxes = [[None, None], [([2] * 4, None), (None, [5, 6, 2**40])], [None, (None, None, [1, -3, 0], None)]]
    lo, hi, nlo, nhi = bx.box_planes(table, boxes)
    assert all(a.dtype == np.int32 and a.shape == (3, 7) for a in (lo, hi, nlo, nhi))
    assert lo.tolist() == [[0] * 7, [2] * 4 + [0] * 3, [0] * 7]
    assert hi.tolist() == [[IMAX] * 7, [IMAX] * 4 + [5, 6, IMAX], [IMAX] * 7]
    assert nlo.tolist() == [[0] * 7, [0] * 7, [0] * 4 + [1, 0, 0]]  # a negative n_min is written as "no bound"
    assert (nhi == IMAX).all()
    lo, hi, nlo, nhi = bx.box_planes(table, boxes[:2])  # no box has an n list: no n planes
    assert nlo is None and nhi is None and lo.shape == (2, 7)


# ------------------------------------------------------------------ the C surface (include/halda_boxes.h)
BOXES_HEADER = REPO / "include" / "halda_boxes.h"
NEW = ("halda_solve_fleets_boxes", "halda_solve_fleets_boxes_host", "halda_last_boxes_route", "halda_set_boxes_path")


def boxes_declarations():
    """name -> (return type, [parameter declarations]) of every function halda_boxes.h itself declares."""
    text = re.sub(r"/\*.*?\*/", "", BOXES_HEADER.read_text(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^\s*(int|int64_t|void)\s+\**(halda_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        out[name] = (ret, [q.strip() for q in " ".join(params.split()).split(",")])
    return out


def test_boxes_header_matches_the_binding():
    """halda_boxes.h against _abi.BOXES_PROTOTYPES, as test_abi.py holds halda.h to _abi.PROTOTYPES: the same
    names, every return type and arity, a scalar parameter exactly its ctypes type, a pointer to a struct of either
    header POINTER of its class, every other pointer some pointer type. halda.h's own tables do not hold them."""
    decl = boxes_declarations()
    assert sorted(decl) == sorted(_abi.BOXES_PROTOTYPES) == sorted(NEW)
    assert not set(decl) & set(_abi.PROTOTYPES) and not set(_abi.BOXES_STRUCTS) & set(_abi.STRUCTS)
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    struct = {cname: cls for cls, cname in {**_abi.STRUCTS, **_abi.BOXES_STRUCTS}.items()}
    for name, (ret, params) in decl.items():
        got_ret, got_args = _abi.BOXES_PROTOTYPES[name]
        assert ret == "int" and got_ret is ctypes.c_int and len(got_args) == len(params), name
        for d, got in zip(params, got_args):
            base = [w for w in d.replace("*", " ").split() if w != "const"][0]
            if "*" not in d:
                assert got is scalar[base], (name, d)
            elif base in struct:
                assert d.count("*") == 1 and got is ctypes.POINTER(struct[base]), (name, d)
            else:
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, d)
    assert {"const halda_boxes *boxes"} <= set(decl["halda_solve_fleets_boxes"][1])
    text = BOXES_HEADER.read_text()
    assert '#include "halda.h"' in text and "HALDA_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_boxes_struct_layout_matches_the_compiled_header(tmp_path):
    """sizeof(halda_boxes) and offsetof of every field, printed by a C program compiled against halda_boxes.h."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    m = re.search(r"typedef struct halda_boxes \{(.*?)\} halda_boxes;", BOXES_HEADER.read_text(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()
    assert body == ["int32_t", "n_box;", "const", "int32_t", "*w_min,", "*w_max,", "*n_min,", "*n_max;"]
    fields = [f[0] for f in HaldaBoxesC._fields_]
    assert fields == ["n_box", "w_min", "w_max", "n_min", "n_max"]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "halda_boxes.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(halda_boxes));']
    lines += [f'    printf("%zu\\n", offsetof(halda_boxes, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", str(BOXES_HEADER.parent), "-o", str(exe), str(src)], check=True,
                   capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(HaldaBoxesC)] + [getattr(HaldaBoxesC, f).offset for f in fields] == [40, 0, 8, 16, 24, 32]


def test_library_and_binding_export_the_new_symbols():
    raw = ctypes.CDLL(str(lh.LIB_PATH))
    lib = lh.load_library(lh.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        fn = getattr(lib, name)  # load_library declared it: no ctypes defaults
        assert fn.restype is _abi.BOXES_PROTOTYPES[name][0] and list(fn.argtypes) == _abi.BOXES_PROTOTYPES[name][1], name
    raw.halda_set_boxes_path.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert raw.halda_set_boxes_path(None, 1) == -22
    raw.halda_last_boxes_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert raw.halda_last_boxes_route(None, None) == -22
    assert lh.ROUTES["boxes"] == ("none", "register", "loop", "tables")
    import distilp.solver as alias
    import distilp_amd.solver as pkg

    for name in ("halda_solve_boxes", "halda_solve_boxes_batch", "reload_caps", "halda_reload_frontier", "ReloadPoint"):
        assert getattr(alias, name) is getattr(pkg, name) is getattr(bx, name)
        assert name in pkg.__all__


# ------------------------------------------------------------------ the reload frontier's host half
def plan(w, obj):
    return HALDAResult(w=w, n=[0] * len(w), k=1, obj_value=obj, sets={"M1": [], "M2": [], "M3": list(range(len(w)))})


def test_reload_frontier_takes_a_strict_running_minimum(monkeypatch, llama_online_model):
    """A stubbed halda_solve_boxes: the boxes it is handed, and what the points make of its answers."""
    model = llama_online_model.model_copy(update={"L": 8})
    group = float(int(model.b_layer))

    class Dev:
        def __init__(self, s):
            self.s_disk = s

    devs = [Dev(2.0), Dev(1.0)]
    seen = {}
    # each device may gain 3: t = 0, 1/2, 1 (= 2/2 = 1/1), 3/2, 2, 3. Answers: pinned, better, equal (keeps the
    # previous plan), worse by a re-ordering of near-equal objectives (keeps it too), best, equal again
    answers = [plan([4, 4], 10.0), plan([5, 3], 9.0), plan([3, 5], 9.0), plan([6, 2], 9.5), plan([7, 1], 8.0),
               plan([6, 2], 8.0), plan([7, 1], 8.0)]

    def fake(devs_, model_, boxes, ks, kv_bits, device):
        seen["boxes"], seen["ks"] = boxes, ks
        return answers

    monkeypatch.setattr(bx, "halda_solve_boxes", fake)
    pts = bx.halda_reload_frontier(devs, model, (1, [4, 4], [0, 0]))
    assert seen["ks"] == [1]
    assert seen["boxes"] == [(None, [4, 4]), (None, [5, 4]), (None, [6, 5]), (None, [7, 5]), (None, [7, 6]),
                             (None, [7, 7]), None]
    assert [p.seconds for p in pts] == [0.0, 0.5 * group, group, 1.5 * group, 2.0 * group, 3.0 * group]
    assert [p.caps for p in pts] == [[0, 0], [1, 0], [2, 1], [3, 1], [3, 2], [3, 3]]
    assert [p.plan.w for p in pts] == [[4, 4], [5, 3], [5, 3], [5, 3], [7, 1], [7, 1]]
    assert [p.obj_value for p in pts] == [10.0, 9.0, 9.0, 9.0, 8.0, 8.0]
    assert [p.gained for p in pts] == [[0, 0], [1, 0], [1, 0], [1, 0], [3, 0], [3, 0]]
    assert [p.seconds_used for p in pts] == [0.0, 0.5 * group, 0.5 * group, 0.5 * group, 1.5 * group, 1.5 * group]
    assert [p.regret for p in pts] == [2.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert all(p.seconds_used <= p.seconds for p in pts)
    # a cut in seconds becomes reload_caps' cut in seconds per layer-byte
    answers[:] = [plan([4, 4], 10.0), plan([5, 3], 9.0), None]
    pts = bx.halda_reload_frontier(devs, model, (1, [4, 4], [0, 0]), max_seconds=0.75 * group)
    assert [p.seconds for p in pts] == [0.0, 0.5 * group] and pts[-1].regret == math.inf
    answers[:] = [None, None, plan([7, 1], 8.0)]  # no plan inside a box: no plan, inf
    pts = bx.halda_reload_frontier(devs, model, (1, [4, 4], [0, 0]), max_points=2)
    assert [(p.plan, p.obj_value, p.regret, p.gained, p.seconds_used) for p in pts] == [(None, math.inf, math.inf,
                                                                                        [0, 0], 0.0)] * 2


@pytest.mark.parametrize("M,k,s", RELOAD_CASES)
def test_reload_cases_improve_at_an_interior_point(llama_online_model, M, k, s):
    """The exact oracle on the first points of the GPU test's cases: point 0 is feasible and some interior point is
    strictly better (by far more than the 1e-9 the GPU's objective may differ from the oracle's)."""
    model = llama_online_model
    devs, w0 = gc.list_case(model, M, k, s)
    W = int(model.L) // k
    t, caps = bx.reload_caps(w0, [float(d.s_disk) for d in devs], W, max_points=8)
    objs = []
    for row in caps:
        b = ([1] * M, [a + int(c) for a, c in zip(w0, row)], [0] * M, [IMAX] * M)
        st, _, _, obj, _ = xc.exact_answer(model, devs, k, b)
        assert st == 0
        objs.append(obj)
    assert all(b <= a + 1e-9 * abs(a) for a, b in zip(objs, objs[1:]))
    assert min(objs[1:]) < objs[0] - 1e-6 * abs(objs[0])


# ------------------------------------------------------------------ the CLI
def test_cli_parses_reload_frontier():
    p = cli._parser()
    a = p.parse_args(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--reload-frontier", "2.5"])
    assert a.reload_frontier == 2.5
    a = p.parse_args(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--reload-frontier"])
    assert a.reload_frontier == math.inf
    assert p.parse_args(["--profile", "hermes_70b"]).reload_frontier is None
    with pytest.raises(SystemExit):
        cli.main(["--profile", "hermes_70b", "--reload-frontier", "2"])  # needs the plan to reload from
    with pytest.raises(SystemExit):
        cli.main(["--profile", "hermes_70b", "--evaluate-solution", "s.json", "--reload-frontier", "-2"])


def test_reload_lines_format(monkeypatch):
    pts = [bx.ReloadPoint(0.0, [0, 0], plan([3, 3], 10.0), 10.0, [0, 0], 0.0, 2.0),
           bx.ReloadPoint(1.5, [1, 0], plan([4, 2], 8.0), 8.0, [1, 0], 1.25, 0.0),
           bx.ReloadPoint(2.0, [1, 1], None, math.inf, [0, 0], 0.0, math.inf)]
    seen = []
    monkeypatch.setattr(bx, "halda_reload_frontier", lambda *a, **k: seen.append((a, k)) or pts)
    lines = cli.reload_lines(["d0", "d1"], "model", (1, [3, 3], [0, 0]), 2.0)
    assert lines == ["reload 0: seconds=0.000000, obj=10.000000, regret=2.000000, gained=[0, 0]",
                     "reload 1: seconds=1.500000, obj=8.000000, regret=0.000000, gained=[1, 0]",
                     "reload 2: infeasible"]
    assert seen == [((["d0", "d1"], "model", (1, [3, 3], [0, 0]), 2.0), {"kv_bits": "4bit"})]
