"""Sub-fleets under boxes without a GPU: the C surface (include/halda_subfleets_boxed.h against the binding, as
tests/test_boxes.py holds halda_boxes.h) and the Python argument errors, raised before any packing or library call."""

import ctypes
import re
import shutil
import subprocess

import pytest

from distilp_amd.solver import _abi
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver import halda_leave_one_out, halda_select_devices, halda_solve_subfleets_bounded
from distilp_amd.solver._abi import HaldaSubBoxesC

from . import bounds_cases as bc
from .conftest import REPO

HEADER = REPO / "include" / "halda_subfleets_boxed.h"
NEW = ("halda_solve_subfleets_boxed", "halda_solve_subfleets_boxed_host", "halda_last_subfleets_boxed_route",
       "halda_set_subfleets_boxed_path")


def test_header_matches_the_binding():
    """Names, return types, arity, a scalar parameter exactly its ctypes type, a pointer to a struct POINTER of its
    class, every other pointer some pointer type; halda.h's and halda_boxes.h's tables do not hold them."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decl = {name: [q.strip() for q in " ".join(params.split()).split(",")]
            for name, params in re.findall(r"^\s*int\s+(halda_\w+)\s*\(([^)]*)\)\s*;", text, re.M)}
    assert sorted(decl) == sorted(_abi.SUBBOX_PROTOTYPES) == sorted(NEW)
    assert not set(decl) & (set(_abi.PROTOTYPES) | set(_abi.BOXES_PROTOTYPES))
    assert not set(_abi.SUBBOX_STRUCTS) & (set(_abi.STRUCTS) | set(_abi.BOXES_STRUCTS))
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    struct = {cname: cls for cls, cname in {**_abi.STRUCTS, **_abi.SUBBOX_STRUCTS}.items()}
    for name, params in decl.items():
        ret, args = _abi.SUBBOX_PROTOTYPES[name]
        assert ret is ctypes.c_int and len(args) == len(params), name
        for d, got in zip(params, args):
            base = [w for w in d.replace("*", " ").split() if w != "const"][0]
            if "*" not in d:
                assert got is scalar[base], (name, d)
            elif base in struct:
                assert d.count("*") == 1 and got is ctypes.POINTER(struct[base]), (name, d)
            else:
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, d)
    assert {"const halda_sub_boxes *boxes", "const halda_subfleets *items"} <= set(decl["halda_solve_subfleets_boxed"])
    assert '#include "halda_boxes.h"' in text and "HALDA_ABI_VERSION" not in text
    assert lh.ROUTES["subfleets_boxed"] == ("none", "register", "expand", "tables")


def test_struct_layout_matches_the_compiled_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = [f[0] for f in HaldaSubBoxesC._fields_]
    assert fields == ["n_box", "w_min", "w_max", "n_min", "n_max", "item_box"]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "halda_subfleets_boxed.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(halda_sub_boxes));']
    lines += [f'    printf("%zu\\n", offsetof(halda_sub_boxes, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", str(HEADER.parent), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(HaldaSubBoxesC)] + [getattr(HaldaSubBoxesC, f).offset for f in fields]
    assert got == [48, 0, 8, 16, 24, 32, 40]


def test_library_and_packages_export_the_new_symbols():
    raw = ctypes.CDLL(str(lh.LIB_PATH))
    lib = lh.load_library(lh.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.restype is _abi.SUBBOX_PROTOTYPES[name][0] and list(fn.argtypes) == _abi.SUBBOX_PROTOTYPES[name][1]
    assert lib.halda_set_subfleets_boxed_path(None, 1) == -22 and lib.halda_version() == 3
    import distilp.solver as alias
    import distilp_amd.solver as pkg

    assert "halda_solve_subfleets_bounded" in pkg.__all__
    assert alias.halda_solve_subfleets_bounded is pkg.halda_solve_subfleets_bounded


BOX4 = (None, [5, 5, 5, 5])
BAD_CALLS = [
    # (items, boxes, exception, text): boxes as halda_solve_boxes_batch refuses them, items as halda_solve_subfleets
    ([(0, [0, 1])], [], ValueError, "empty"),
    ([(0, [0, 1])], [[BOX4, None]], ValueError, "2 bounds for 1 fleets"),
    ([(0, [0, 1])], [[(None, [5, 5, 5])]], ValueError, "3 entries"),
    ([(0, [0, 1])], [[([0, 1, 1, 1], None)]], ValueError, ">= 1"),
    ([(0, [0, 1], 1)], [[BOX4]], ValueError, "box 1"),
    ([(0, [0, 1], True)], [[BOX4]], ValueError, "box True"),
    ([(0,)], [[BOX4]], ValueError, "neither"),
    ([(0, [])], [[BOX4]], ValueError, "empty device list"),
    ([(0, [4])], [[BOX4]], IndexError, "device index 4"),
    ([(1, [0])], [[BOX4]], IndexError, "fleet index 1"),
]


@pytest.mark.parametrize("items,boxes,exc,text", BAD_CALLS)
def test_argument_errors_come_before_any_packing(monkeypatch, llama_online_model, items, boxes, exc, text):
    def no_call(*a, **k):
        raise AssertionError("packed or reached the library")

    monkeypatch.setattr(sf, "fleet_table", no_call)
    monkeypatch.setattr(sf, "get_context", no_call)
    with pytest.raises(exc, match=text):
        halda_solve_subfleets_bounded([list(bc.devices(4, 0))], llama_online_model, items, boxes)


def test_the_bounds_keyword_checks_its_box_first(monkeypatch, llama_online_model):
    def no_call(*a, **k):
        raise AssertionError("packed or reached the library")

    monkeypatch.setattr(sf, "fleet_table", no_call)
    devs = list(bc.devices(4, 0))
    with pytest.raises(ValueError, match="3 entries"):
        halda_leave_one_out(devs, llama_online_model, bounds=(None, [5, 5, 5]))
    with pytest.raises(ValueError, match="3 entries"):
        halda_select_devices(devs, llama_online_model, bounds=(None, [5, 5, 5]))
