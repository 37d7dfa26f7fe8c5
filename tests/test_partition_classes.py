"""Replica partitioning by device class without a GPU: the classes of a packed table, the gate's errors, the C
surface (include/halda_partition_classes.h against the binding) and the scratch figure."""

import ctypes
import re

import pytest

from distilp_amd.solver import _abi
from distilp_amd.solver import partition as pt
from distilp_amd.solver.fleets import fleet_table

from . import bounds_cases as bc
from .conftest import REPO

HEADER = REPO / "include" / "halda_partition_classes.h"


def test_device_classes_by_bitwise_row_equality(llama_online_model):
    h, a, b, c = bc.devices(4, 0)  # h is the only is_head device
    table = fleet_table([[a, b, b, a, c, a], [a, a.model_copy(update={"is_head": True}), a], [h, a, b, c]],
                        llama_online_model)
    cls, counts, order = pt.device_classes(table, 0)
    assert (cls.tolist(), counts.tolist(), order.tolist()) == ([0, 1, 1, 0, 2, 0], [3, 2, 1], [0, 3, 5, 1, 2, 4])
    cls, counts, order = pt.device_classes(table, 1)  # the only difference is is_head
    assert (cls.tolist(), counts.tolist(), order.tolist()) == ([0, 1, 0], [2, 1], [0, 2, 1])
    cls, counts, order = pt.device_classes(table, 2)
    assert (cls.tolist(), counts.tolist(), order.tolist()) == ([0, 1, 2, 3], [1] * 4, [0, 1, 2, 3])


@pytest.mark.parametrize("counts, groups, match", [
    ([[1] * 9], 2, "at most 8 classes, fleet 0 has 9"),
    ([[4], [129, 128]], 2, "at most 256 devices, fleet 1 has 257"),
    ([[15, 15, 15, 15, 16]], 2, "2\\^20 codes, fleet 0 has 1114112"),  # 16^4 * 17
    ([[15] * 5], 2, "2\\^32 pair evaluations"),  # 16^5 = 2^20 codes, 136^5 pairs
    ([[2, 1]], 4, "beyond the 3 devices"),
    ([[2, 1]], 9, "1..8"),
])
def test_gate_errors(counts, groups, match):
    with pytest.raises(ValueError, match=match):
        pt.check_gate_classes(counts, groups, "max")
    assert pt.check_gate_classes([[16] * 4, [128, 128]], 8, "sum") == 1


def test_routes(monkeypatch, llama_online_model):
    d4 = list(bc.devices(4, 0))
    with pytest.raises(ValueError, match="route"):
        pt.halda_partition_frontier(d4, llama_online_model, 2, route="codes")
    monkeypatch.setattr(pt, "fleet_table", lambda *a, **k: pytest.fail("reached the packer"))
    for route in ("masks", None):  # the default is today's call: same gate, same error
        with pytest.raises(ValueError, match="at most 20 devices, fleet 0 has 24"):
            pt.halda_partition(d4 * 6, llama_online_model, 2, **({"route": route} if route else {}))
    with pytest.raises(ValueError, match="criterion"):
        pt.halda_partition_frontier(d4 * 6, llama_online_model, 2, "min", route="classes")


def test_header_matches_the_binding():
    """halda_partition_classes.h against _abi.PARTITION_CLASSES_PROTOTYPES, as tests/test_partition.py holds
    halda_partition.h: names, result types and arity, scalars exactly, struct pointers by class, field order."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decl = {name: (ret, [q.strip() for q in " ".join(params.split()).split(",")]) for ret, name, params in
            re.findall(r"^\s*(int|int64_t|void)\s+\**(halda_\w+)\s*\(([^)]*)\)\s*;", text, re.M)}
    protos = _abi.PARTITION_CLASSES_PROTOTYPES
    assert sorted(decl) == sorted(protos)
    assert not set(decl) & (set(_abi.PROTOTYPES) | set(_abi.BOXES_PROTOTYPES) | set(_abi.WIDE_PROTOTYPES)
                            | set(_abi.PARTITION_PROTOTYPES))
    scalar = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    struct = {cname: cls for cls, cname in {**_abi.STRUCTS, **_abi.PARTITION_CLASSES_STRUCTS}.items()}
    for name, (ret, params) in decl.items():
        got_ret, got_args = protos[name]
        assert got_ret is scalar[ret] and len(got_args) == len(params), name
        for d, got in zip(params, got_args):
            base = [w for w in d.replace("*", " ").split() if w != "const"][0]
            if "*" not in d:
                assert got is scalar[base], (name, d)
            elif base in struct:
                assert d.count("*") == 1 and got is ctypes.POINTER(struct[base]), (name, d)
            else:
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, d)
    for cls, cname in _abi.PARTITION_CLASSES_STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, re.S).group(1)
        assert re.findall(r"(\w+);", body) == [f[0] for f in cls._fields_], cname
    assert '#include "halda_partition.h"' in text and "HALDA_ABI_VERSION" not in text


def test_partition_classes_bytes_at_and_outside_the_gate():
    """Per code: val 8, k 4, two best planes 16, and 4 per arg plane of the levels 2 .. R."""
    assert pt.partition_classes_bytes([16] * 4, 4) == 17 ** 4 * (28 + 4 * 3)
    assert pt.partition_classes_bytes([128, 128], 8) == 129 * 129 * 56
    assert [pt.partition_classes_bytes(c, r) for c, r in (([1] * 9, 2), ([129, 128], 2), ([15, 15, 15, 15, 16], 2),
                                                          ([15] * 5, 2), ([4, 0], 2), ([4], 0), ([4], 9))] == [-1] * 7
    assert pt.partition_classes_bytes([3] * 8, 2) == 4 ** 8 * 32 and pt.partition_classes_bytes([255], 2) == 256 * 32
