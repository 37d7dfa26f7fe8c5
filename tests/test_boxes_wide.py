"""Route "wide" of the many-boxes entry without a GPU: its gate (raised before packing or any library call), the
slice figures against the library's, and include/halda_boxes_wide.h against the binding's table."""

import ctypes
import re

import pytest

from distilp_amd.solver import _abi
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import bounds as bd
from distilp_amd.solver import boxes as bx

from .conftest import REPO

HEADER = REPO / "include" / "halda_boxes_wide.h"


@pytest.mark.parametrize("shape", [dict(max_devices=257), dict(n_box=0), dict(ks=list(range(1, 66))),
                                   dict(min_devices=0), dict(n_box=65536), dict(n_box=65535, n_fleets=65536),
                                   dict(L=30000)])
def test_gate_raises_outside_it(shape):
    ok = dict(max_devices=256, min_devices=1, n_box=8, n_fleets=2, ks=[1, 2, 4], L=320)
    bx.check_gate_wide(**ok)
    with pytest.raises(ValueError):
        bx.check_gate_wide(**{**ok, **shape})


def test_gate_is_checked_before_packing(monkeypatch, llama_online_model):
    """257 devices, no boxes, 65 k: a ValueError with the packer and the library out of reach."""
    def boom(*a, **k):
        raise AssertionError("packed or called before the gate")

    monkeypatch.setattr(bx, "fleet_table", boom)
    monkeypatch.setattr(bx, "get_context", boom)
    model = llama_online_model
    for M, boxes, ks in ((257, [None], [1]), (3, [], [1]), (3, [None], list(range(1, 66)))):
        with pytest.raises(ValueError):
            bx.halda_solve_boxes([None] * M, model, boxes, ks, "4bit", route="wide")
    with pytest.raises(ValueError):
        bd.halda_solve_bounded([None] * 257, model, k_candidates=[1], kv_bits="4bit", route="wide")
    with pytest.raises(ValueError, match="route"):
        bx.halda_solve_boxes([None] * 3, model, [None], [1], "4bit", route="tables")


@pytest.mark.parametrize("M,max_R,kc", [(16, 79, True), (70, 90, False), (256, 64, True), (3, 317, False)])
def test_slice_figures_equal_the_librarys(M, max_R, kc):
    lib = lh.load_library()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert lib.halda_boxes_wide_bytes(M, max_R, int(kc), ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == bx.boxes_wide_bytes(M, max_R, kc)
    assert lib.halda_boxes_wide_bytes(0, 1, 0, ctypes.byref(a), ctypes.byref(b)) == -22


def test_header_matches_the_binding():
    """halda_boxes_wide.h against _abi.BOXES_WIDE_PROTOTYPES, as tests/test_boxes.py holds halda_boxes.h to its
    table: the same names, return types and arity; scalars exactly, struct pointers POINTER of their class."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decl = {name: [q.strip() for q in " ".join(params.split()).split(",")]
            for name, params in re.findall(r"^\s*int\s+(halda_\w+)\s*\(([^)]*)\)\s*;", text, re.M)}
    assert sorted(decl) == sorted(_abi.BOXES_WIDE_PROTOTYPES) and len(decl) == 3
    assert not set(decl) & (set(_abi.PROTOTYPES) | set(_abi.BOXES_PROTOTYPES) | set(_abi.WIDE_PROTOTYPES))
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    struct = {cname: cls for cls, cname in {**_abi.STRUCTS, **_abi.BOXES_STRUCTS}.items()}
    for name, params in decl.items():
        ret, args = _abi.BOXES_WIDE_PROTOTYPES[name]
        assert ret is ctypes.c_int and len(args) == len(params), name
        for d, got in zip(params, args):
            base = [w for w in d.replace("*", " ").split() if w != "const"][0]
            if "*" not in d:
                assert got is scalar[base], (name, d)
            elif base in struct:
                assert got is ctypes.POINTER(struct[base]), (name, d)
            else:
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, d)
    assert '#include "halda_boxes.h"' in text and "HALDA_ABI_VERSION" not in text
    lib = lh.load_library()
    assert all(getattr(lib, n).argtypes == _abi.BOXES_WIDE_PROTOTYPES[n][1] for n in decl)
