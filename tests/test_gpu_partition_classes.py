"""Replica partitioning by device class on the GPU (libhalda halda_solve_partition_classes): the raw frontier equals
the mask route's values on fleets both admit, and equals, bit for bit, a plain NumPy programme over count vectors on
the raw obj_value / best_k that halda_solve_subfleets (the C entry) writes for every code's class-order list."""

import ctypes
import math
from functools import lru_cache

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_partition, halda_partition_frontier, halda_solve_subfleets
from distilp_amd.solver import partition as pt
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver.fleets import HaldaFleetResultC, fleet_table, model_struct

from . import pressure_cases as pc
from . import tied_cases as tc
from .test_gpu_partition import PRESSURED
from .test_gpu_subfleets import KS80, _torch, _upload, fleet

pytestmark = pytest.mark.gpu


def by_counts(counts, seed, kinds=None):
    """A class-sorted fleet: counts[c] copies of kind c."""
    kinds = kinds or fleet(len(counts), seed)
    return [kinds[c] for c, n in enumerate(counts) for _ in range(n)]


def interleaved():
    h, a, b = fleet(3, 9501)  # h is the only is_head device: a group without it is headed by its first device
    return [a, b, b, a, h, a]


def pressured():
    d = pc.devices(*PRESSURED)  # device 0 cannot hold a pipeline alone
    return by_counts((3, 3), 0, d[:2])


# name: (fleet, model, R)
FLEETS = {
    "interleaved": lambda: (interleaved(), pc.our_model(), 4),
    "3x8": lambda: (by_counts((8, 8, 8), 9524), pc.our_model(), 4),  # 729 codes: LDS source; S = full has 648 candidates
    "4x9": lambda: (by_counts((9, 9, 9, 9), 9536), pc.our_model(), 3),  # 10,000 codes: the first global-source size
    "pressured": lambda: (pressured(), pc.our_model(), 4),
    "2x50": lambda: (by_counts((50, 50), 9600), tc.model(80), 4),  # more devices than layers
}


def reference(val, counts, R, criterion):
    """The recurrence over count vectors on val[code] (val[0] unused), one lexicographic minimum per S: per
    r = 1 .. R the value of the full vector and its group codes by backtrack (None where it is inf)."""
    radix = np.asarray(counts, np.int64) + 1
    stride = np.concatenate([[1], np.cumprod(radix)[:-1]])
    n = int(np.prod(radix))
    digits = (np.arange(n)[:, None] // stride) % radix
    devs = digits.sum(axis=1)
    best, arg = [None, val], [None, None]
    for r in range(2, R + 1):
        cur, a = np.full(n, np.inf), np.zeros(n, np.int64)
        for S in ([n - 1] if r == R else range(1, n)):
            if devs[S] < r:
                continue
            c0 = int(np.flatnonzero(digits[S])[0])
            T = np.flatnonzero((digits[:S] <= digits[S]).all(axis=1) & (digits[:S, c0] >= 1))
            v = val[T] + best[r - 1][S - T] if criterion == "sum" else np.maximum(val[T], best[r - 1][S - T])
            cur[S] = v.min()
            a[S] = T[v == cur[S]][0]  # T ascends: the smallest code among equals
        best.append(cur)
        arg.append(a)
    out = []
    for r in range(1, R + 1):
        v, S, groups = (best[r][n - 1] if devs[n - 1] >= r else np.inf), n - 1, []
        for lvl in range(r, 1, -1) if v < np.inf else ():
            groups.append(int(arg[lvl][S]))
            S -= groups[-1]
        out.append((v, groups + [S] if v < np.inf else None))
    return out


def code_values(table, counts, order, model, parent=0):
    """val and k of every code of fleet `parent` (entry 0 unused): the raw outputs of one halda_solve_subfleets call on
    device arrays over the codes' class-order lists."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    n = math.prod(int(c) + 1 for c in counts)
    items = [(parent, pt._class_groups([code], counts, order)[0]) for code in range(1, n)]
    arrs, fs = _upload(table)
    parent_, sub_off, sub_idx = sf.pack_items(table.sizes(), items)
    d = [torch.from_numpy(a).to(dev) for a in (parent_, sub_off, sub_idx)]
    lens = np.diff(sub_off)
    it = sf.HaldaSubfleetsC(n - 1, int(lens.min()), int(lens.max()), *[t.data_ptr() for t in d])
    k, obj = torch.zeros(n - 1, dtype=torch.int32, device=dev), torch.zeros(n - 1, dtype=torch.float64, device=dev)
    w = torch.zeros(2 * int(sub_off[-1]), dtype=torch.int32, device=dev)
    r = HaldaFleetResultC(k.data_ptr(), obj.data_ptr(), w.data_ptr(), w.data_ptr() + 4 * int(sub_off[-1]), None, None,
                          None, None, None)
    karr, m = np.asarray(KS80, np.int32), model_struct(model, 0.5)
    torch.cuda.synchronize(dev)
    with ctx._lock:
        rc = ctx.lib.halda_solve_subfleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                           karr.ctypes.data, len(KS80), ctypes.byref(r), None)
    assert rc == 0, lh.last_error(ctx.lib)
    torch.cuda.synchronize(dev)
    return np.concatenate([[np.inf], obj.cpu().numpy()]), np.concatenate([[0], k.cpu().numpy()])


def solve_raw(fleets, model, R, criterion):
    table = fleet_table(fleets, model)
    classes = [pt.device_classes(table, f) for f in range(len(fleets))]
    cls = np.concatenate([c[0] for c in classes])
    return table, classes, cls, pt.solve_partition_classes_table(table, cls, model, KS80, 0.5, R,
                                                                 pt.CRITERIA.index(criterion))


@lru_cache(maxsize=None)
def solved(name, criterion):
    """(raw frontier, val, k, counts, R) of a named fleet: solved once, shared, read only."""
    devs, model, R = FLEETS[name]()
    table, classes, _, raw = solve_raw([devs], model, R, criterion)
    val, ks = code_values(table, classes[0][1], classes[0][2], model)
    return raw, val, ks, classes[0][1], R


def check_fleet(raw, f, val, ks, counts, R, criterion):
    """Fleet f of a raw frontier against the reference on `val`: every point's bits, codes, obj and k."""
    status, value, gcode, gobj, gk = raw
    for r, (v, groups) in enumerate(reference(val, counts, R, criterion), 1):
        what = (criterion, r)
        if groups is None:
            assert status[f, r - 1] == lh.STATUS_INFEASIBLE and value[f, r - 1] == math.inf, what
            assert not gcode[f, r - 1].any() and (gobj[f, r - 1] == math.inf).all() and not gk[f, r - 1].any(), what
            continue
        assert status[f, r - 1] == lh.STATUS_OPTIMAL, what
        assert np.float64(v).tobytes() == value[f, r - 1].tobytes(), (what, v, value[f, r - 1])
        assert gcode[f, r - 1, :r].tolist() == groups and not gcode[f, r - 1, r:].any(), (what, groups)
        assert val[groups].tobytes() == gobj[f, r - 1, :r].tobytes(), what
        assert gk[f, r - 1, :r].tolist() == ks[groups].tolist(), what
        assert (gobj[f, r - 1, r:] == math.inf).all() and not gk[f, r - 1, r:].any(), what


@pytest.mark.parametrize("criterion", pt.CRITERIA)
@pytest.mark.parametrize("counts", [(4, 3), (2, 2, 2, 2), (8,), (1, 1, 1, 1, 1)])
def test_values_equal_the_mask_route_bit_for_bit(counts, criterion):
    """The groups may differ under the tie rule; the statuses and values may not. All-distinct: codes are masks."""
    devs, model = by_counts(counts, 9400 + len(counts)), pc.our_model()
    table, _, _, raw = solve_raw([devs], model, 4, criterion)
    masks = pt.solve_partition_table(table, model, KS80, 0.5, 4, pt.CRITERIA.index(criterion))
    assert raw[0].tobytes() == masks[0].tobytes() and raw[1].tobytes() == masks[1].tobytes(), (raw[1], masks[1])
    if max(counts) == 1:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, masks))


@pytest.mark.parametrize("criterion", pt.CRITERIA)
@pytest.mark.parametrize("name", ["interleaved", "3x8", "4x9", "pressured"])
def test_frontier_equals_the_recurrence_over_count_vectors_bit_for_bit(name, criterion):
    raw, val, ks, counts, R = solved(name, criterion)
    if name == "pressured":
        assert val[1] == math.inf and val[4] < math.inf  # one starved device alone; one of the other class
    check_fleet(raw, 0, val, ks, counts, R, criterion)


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_more_devices_than_layers(criterion):
    raw, val, ks, counts, R = solved("2x50", criterion)
    assert raw[0][0, 0] == lh.STATUS_INFEASIBLE and lh.STATUS_OPTIMAL in raw[0][0].tolist()
    check_fleet(raw, 0, val, ks, counts, R, criterion)


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_mixed_batch_and_device_entry(criterion):
    """A batch of two class structures equals the single-fleet calls; the device entry equals the host entry."""
    torch, dev = _torch()
    model, R, fleets = pc.our_model(), 4, [interleaved(), by_counts((2, 5), 9702)]
    table, _, cls, both = solve_raw(fleets, model, R, criterion)
    for f, devs in enumerate(fleets):
        one = solve_raw([devs], model, R, criterion)[3]
        assert all(a[f].tobytes() == b[0].tobytes() for a, b in zip(both, one)), (criterion, f)
    ctx = lh.get_context(0)
    arrs, fs = _upload(table)
    n = table.n_fleets * R
    o = [torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7.0, dtype=torch.float64, device=dev),
         torch.full((8 * n,), -7, dtype=torch.int32, device=dev),
         torch.full((8 * n,), -7.0, dtype=torch.float64, device=dev),
         torch.full((8 * n,), -7, dtype=torch.int32, device=dev)]
    fr = pt.HaldaPartitionClassesFrontierC(*[t.data_ptr() for t in o])
    off = np.ascontiguousarray(table.dev_off, np.int64)
    part = pt.HaldaPartitionClassesC(R, pt.CRITERIA.index(criterion), cls.ctypes.data, off.ctypes.data)
    karr, m = np.asarray(KS80, np.int32), model_struct(model, 0.5)
    torch.cuda.synchronize(dev)
    with ctx._lock:
        rc = ctx.lib.halda_solve_partition_classes(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
                                                   karr.ctypes.data, len(KS80), ctypes.byref(fr), None)
    assert rc == 0, lh.last_error(ctx.lib)
    torch.cuda.synchronize(dev)
    for a, b in zip(o, both):
        assert a.cpu().numpy().tobytes() == b.tobytes(), criterion


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_python_entries(criterion):
    model = pc.our_model()
    devs = [d for _ in range(8) for d in fleet(3, 9524)]  # 24 devices, the three kinds interleaved
    pts = halda_partition_frontier(devs, model, 3, criterion, kv_bits="4bit", route="classes")
    assert any(p.groups is not None for p in pts)
    for p in pts:
        if p.groups is None:
            continue
        assert sorted(i for g in p.groups for i in g) == list(range(24))
        for g, res in zip(p.groups, p.results):
            assert res == halda_solve_subfleets([devs], model, [(0, g)], kv_bits="4bit")[0], g
        assert p.value == pt.combine([x.obj_value for x in p.results], criterion)
    assert halda_partition_frontier(devs, model, 3, criterion, kv_bits="4bit", route="auto") == pts
    assert halda_partition(devs, model, 3, criterion, kv_bits="4bit", route="classes") == pts[-1]
    d8 = by_counts((4, 4), 9802)
    assert (halda_partition_frontier(d8, model, 3, criterion, kv_bits="4bit", route="auto")
            == halda_partition_frontier(d8, model, 3, criterion, kv_bits="4bit"))
    with pytest.raises(RuntimeError, match="No feasible partition into 6 groups"):
        halda_partition(pressured(), model, 6, criterion, kv_bits="4bit", route="classes")
