"""Exact replica partitioning without a GPU: the gate's errors before any packing, the C surface
(include/halda_partition.h against the binding) and the scratch figure."""

import ctypes
import re

import pytest

from distilp_amd.solver import _abi
from distilp_amd.solver import partition as pt

from . import bounds_cases as bc
from .conftest import REPO

HEADER = REPO / "include" / "halda_partition.h"


def test_gate_and_criterion_raise_before_packing(monkeypatch, llama_online_model):
    def absent(*a, **k):
        raise AssertionError("reached the packer or the library")

    monkeypatch.setattr(pt, "get_context", absent)
    monkeypatch.setattr(pt, "fleet_table", absent)
    d4 = list(bc.devices(4, 0))
    for groups, criterion, match in ((0, "max", "1..8"), (9, "max", "1..8"), (5, "sum", "beyond the 4 devices"),
                                     (2, "min", "criterion"), (2.0, "max", "not an integer")):
        with pytest.raises(ValueError, match=match):
            pt.halda_partition_frontier(d4, llama_online_model, groups, criterion)
    with pytest.raises(ValueError, match="at most 20 devices, fleet 1 has 21"):
        pt.halda_partition_frontier_batch([d4, d4 * 5 + d4[:1]], llama_online_model, 2)
    with pytest.raises(ValueError, match="beyond"):
        pt.halda_partition(d4, llama_online_model, 5)
    assert pt.check_gate([3, 7], 4, "sum") == 1 and pt.check_gate([20], 8, "max") == 0


def test_header_matches_the_binding():
    """halda_partition.h against _abi.PARTITION_PROTOTYPES: the same names, every result type and arity, a scalar
    parameter exactly its ctypes type, a pointer to a struct of either header POINTER of its class."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decl = {name: (ret, [q.strip() for q in " ".join(params.split()).split(",")]) for ret, name, params in
            re.findall(r"^\s*(int|int64_t|void)\s+\**(halda_\w+)\s*\(([^)]*)\)\s*;", text, re.M)}
    assert sorted(decl) == sorted(_abi.PARTITION_PROTOTYPES)
    assert not set(decl) & (set(_abi.PROTOTYPES) | set(_abi.BOXES_PROTOTYPES) | set(_abi.WIDE_PROTOTYPES))
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    struct = {cname: cls for cls, cname in {**_abi.STRUCTS, **_abi.PARTITION_STRUCTS}.items()}
    for name, (ret, params) in decl.items():
        got_ret, got_args = _abi.PARTITION_PROTOTYPES[name]
        assert got_ret is scalar[ret] and len(got_args) == len(params), name
        for d, got in zip(params, got_args):
            base = [w for w in d.replace("*", " ").split() if w != "const"][0]
            if "*" not in d:
                assert got is scalar[base], (name, d)
            elif base in struct:
                assert d.count("*") == 1 and got is ctypes.POINTER(struct[base]), (name, d)
            else:
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, d)
    for cls, cname in _abi.PARTITION_STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, re.S).group(1)
        assert re.findall(r"(\w+);", body) == [f[0] for f in cls._fields_], cname
    assert '#include "halda.h"' in text and "HALDA_ABI_VERSION" not in text


def test_partition_bytes_are_the_documented_planes():
    """Per mask: val 8, k 4, two best planes 16, and 4 per arg plane of the levels 2 .. R."""
    assert pt.partition_bytes(13, 4) == (1 << 13) * (8 + 4 + 16 + 4 * 3) == 327680
    assert pt.partition_bytes(20, 8) == (1 << 20) * (8 + 4 + 16 + 4 * 7) == 58720256
    assert [pt.partition_bytes(m, r) for m, r in ((0, 1), (21, 2), (5, 0), (5, 9))] == [-1] * 4
