"""Exact replica partitioning on the GPU (libhalda halda_solve_partition): the frontier's raw values, group masks
and per-group obj / k equal, bit for bit, a plain dynamic programme over the raw obj_value / best_k that
halda_solve_subfleets (the C entry) writes for every mask's list, and the Python entries built on it agree with the
same programme over the exact oracle's values."""

import copy
import ctypes
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

from distilp_amd.common import DeviceProfile
from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_partition, halda_partition_frontier, halda_partition_frontier_batch
from distilp_amd.solver import partition as pt
from distilp_amd.solver.fleets import fleet_table, model_struct
from distilp_amd.synth import synth_fleet

from . import pressure_cases as pc
from . import subsets_cases as sc
from . import tied_cases as tc
from .test_gpu_subfleets import KS80, _torch, _upload, fleet, solve_items_device

pytestmark = pytest.mark.gpu

OPS = {"max": max, "sum": lambda a, b: a + b}
# a memory-pressured fleet (pressure_cases.devices(seed, M, scale)) whose device 0 cannot hold a pipeline alone, by the
# exact oracle on the CPU: with R = M = 5 the points 1 .. 4 have a partition and point 5 (five groups of one) has none
PRESSURED = (0, 5, Fraction(1, 16384))


def reference(val, M, R, op):
    """The recurrence over a dict of Python floats, min on the pair (value, T); per r = 1 .. R the value of the full
    mask and its groups by backtrack (None where it is inf)."""
    full = (1 << M) - 1
    best = [None, {S: (val[S], S) for S in range(1, full + 1)}]
    for r in range(2, R + 1):
        best.append({})
        for S in range(1, full + 1):
            low, c = S & -S, (math.inf, 1 << 32)
            F = x = S ^ low
            while x and bin(S).count("1") >= r:
                x = (x - 1) & F
                c = min(c, (op(val[low | x], best[r - 1][S ^ low ^ x][0]), low | x))
            best[r][S] = c
    out = []
    for r in range(1, R + 1):
        v, S, groups = best[r].get(full, (math.inf, 0))[0] if M >= r else math.inf, full, []
        for lvl in range(r, 1, -1) if v < math.inf else ():
            groups.append(best[lvl][S][1])
            S ^= groups[-1]
        out.append((v, groups + [S] if v < math.inf else None))
    return out


def mask_items(M, parent=0):
    return [(parent, pt.mask_devices(m)) for m in range(1, 1 << M)]


def raw_values(table, model, M, parent=0):
    """val and k of every mask of fleet `parent`: the raw outputs of one halda_solve_subfleets call."""
    o = solve_items_device(table, mask_items(M, parent), model, KS80)
    return ({m: float(o["obj_value"][m - 1]) for m in range(1, 1 << M)},
            {m: int(o["best_k"][m - 1]) for m in range(1, 1 << M)})


def check_fleet(raw, f, val, ks, M, R, criterion):
    """Fleet f of a raw frontier against the reference on `val`: every point's bits, masks, obj and k."""
    status, value, gmask, gobj, gk = raw
    for r, (v, groups) in enumerate(reference(val, M, R, OPS[criterion]), 1):
        what = (criterion, M, r)
        if groups is None:
            assert status[f, r - 1] == lh.STATUS_INFEASIBLE and value[f, r - 1] == math.inf, what
            assert not gmask[f, r - 1].any() and (gobj[f, r - 1] == math.inf).all() and not gk[f, r - 1].any(), what
            continue
        assert status[f, r - 1] == lh.STATUS_OPTIMAL, what
        assert np.float64(v).tobytes() == value[f, r - 1].tobytes(), (what, v, value[f, r - 1])
        assert gmask[f, r - 1, :r].tolist() == groups and not gmask[f, r - 1, r:].any(), (what, groups)
        assert [np.float64(val[g]).tobytes() for g in groups] == [x.tobytes() for x in gobj[f, r - 1, :r]], what
        assert gk[f, r - 1, :r].tolist() == [ks[g] for g in groups], what
        assert (gobj[f, r - 1, r:] == math.inf).all() and not gk[f, r - 1, r:].any(), what


def solve_raw(fleets, model, R, criterion):
    table = fleet_table(fleets, model)
    return table, pt.solve_partition_table(table, model, KS80, 0.5, R, pt.CRITERIA.index(criterion))


@pytest.mark.parametrize("criterion", pt.CRITERIA)
@pytest.mark.parametrize("M", [2, 3, 5])
def test_points_match_the_recurrence_over_the_exact_oracle(M, criterion):
    key = ("synth", 9100 + M, M)
    devs, model, kv, _ = sc.fleet_of(key)
    want = {m: sc.oracle_of(key, tuple(pt.mask_devices(m))) for m in range(1, 1 << M)}
    val = {m: math.inf if o is None else o["obj_value"] for m, o in want.items()}
    R = min(M, 4)
    pts = halda_partition_frontier(devs, model, R, criterion, kv_bits=kv)
    assert len(pts) == R
    for p, (v, groups) in zip(pts, reference(val, M, R, OPS[criterion])):
        assert (p.groups is None) == (groups is None)
        if groups is None:
            continue
        assert abs(p.value - v) <= sc.REL_OBJ * max(1.0, abs(v)), (M, criterion, p.value, v)
        assert sorted(i for g in p.groups for i in g) == list(range(M)) and p.groups[0][0] == 0
        for g, r in zip(p.groups, p.results):
            o = want[sum(1 << i for i in g)]["obj_value"]
            assert abs(r.obj_value - o) <= sc.REL_OBJ * max(1.0, abs(o)), (M, criterion, g)
    assert halda_partition(devs, model, R, criterion, kv_bits=kv) == pts[-1]


@pytest.mark.parametrize("criterion", pt.CRITERIA)
@pytest.mark.parametrize("M", [7, 8, 13, 14])
def test_frontier_equals_the_recurrence_on_the_entry_s_values_bit_for_bit(M, criterion):
    """p - 1 = 6 and 7 at the full mask (one and two steps per lane), the last LDS-source size and the first
    global-source size."""
    devs, model = fleet(M, 9300 + M), pc.our_model()
    table, raw = solve_raw([devs], model, 4, criterion)
    val, ks = raw_values(table, model, M)
    check_fleet(raw, 0, val, ks, M, 4, criterion)


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_homogeneous_fleet_where_nearly_every_value_ties(criterion):
    src = synth_fleet(tc.SEED0, 16)
    devs = [DeviceProfile.model_validate(copy.deepcopy(d)) for d in tc.tied_dicts("copies", src, 0, 8)]
    table, raw = solve_raw([devs], tc.model(), 4, criterion)
    val, ks = raw_values(table, tc.model(), 8)
    assert len(set(val.values())) <= 8  # one value per group size
    check_fleet(raw, 0, val, ks, 8, 4, criterion)


@lru_cache(maxsize=None)
def mixed():
    return [fleet(3, 9403), fleet(7, 9407)]


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_mixed_batch_equals_the_single_fleet_calls(criterion):
    model = pc.our_model()
    _, both = solve_raw(mixed(), model, 4, criterion)
    assert both[0][0, 3] == lh.STATUS_INFEASIBLE and both[1][0, 3] == math.inf and not both[2][0, 3].any()
    for f, devs in enumerate(mixed()):
        _, one = solve_raw([devs], model, min(len(devs), 4), criterion)
        r = one[0].shape[1]
        for a, b in zip(both, one):
            assert a[f, :r].tobytes() == b[0].tobytes(), (criterion, f)
    pts = halda_partition_frontier_batch(mixed(), model, 4, criterion, kv_bits="4bit")
    assert pts[0][3] == pt.PartitionPoint(None, None, math.inf) and pts[1][3].groups is not None


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_pressured_fleet_points_that_need_a_starved_group_are_infeasible(criterion):
    seed, M, scale = PRESSURED
    devs, model = pc.devices(seed, M, scale), pc.our_model()
    table, raw = solve_raw([devs], model, M, criterion)
    val, ks = raw_values(table, model, M)
    assert val[1] == math.inf and all(val[1 << i] < math.inf for i in range(1, M))
    assert raw[0][0].tolist() == [lh.STATUS_OPTIMAL] * 4 + [lh.STATUS_INFEASIBLE]
    check_fleet(raw, 0, val, ks, M, M, criterion)
    with pytest.raises(RuntimeError, match="No feasible partition into 5 groups"):
        halda_partition(devs, model, M, criterion, kv_bits="4bit")


@pytest.mark.parametrize("criterion", pt.CRITERIA)
def test_device_and_host_entries_agree_bit_for_bit(criterion):
    torch, dev = _torch()
    model, R = pc.our_model(), 4
    table, host = solve_raw(mixed(), model, R, criterion)
    ctx = lh.get_context(0)
    arrs, fs = _upload(table)
    n = table.n_fleets * R
    o = [torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7.0, dtype=torch.float64, device=dev),
         torch.full((8 * n,), -7, dtype=torch.int32, device=dev),
         torch.full((8 * n,), -7.0, dtype=torch.float64, device=dev),
         torch.full((8 * n,), -7, dtype=torch.int32, device=dev)]
    fr = pt.HaldaPartitionFrontierC(*[t.data_ptr() for t in o])
    part = pt.HaldaPartitionC(R, pt.CRITERIA.index(criterion))
    karr = np.asarray(KS80, np.int32)
    m = model_struct(model, 0.5)
    torch.cuda.synchronize(dev)
    with ctx._lock:
        rc = ctx.lib.halda_solve_partition(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
                                           karr.ctypes.data, len(KS80), ctypes.byref(fr), None)
    assert rc == 0, lh.last_error(ctx.lib)
    torch.cuda.synchronize(dev)
    for a, b in zip(o, host):
        assert a.cpu().numpy().tobytes() == b.tobytes(), criterion
