"""Every synchronous host entry of libhalda against its device entry, bit for bit, on one tiny ragged table.

Three fleets of 2, 3 and 5 synthetic devices (no array size a multiple of 256 bytes), the L = 80 model,
ks = (4, 20, 40): W = L / k = 20, 4, 2, so k = 20 leaves the 5-device fleet and k = 40 the 3- and 5-device
fleets infeasible. Each host entry is called through ctypes on NumPy arrays and compared with the matching
device entry run on the same table uploaded with torch, in three output layouts:
  dense    x / c with the stride 7 max_devices + 1 (the Python wrappers only ever ask for the compact one);
  compact  x / c through x_off, one instance marked -1;
  bare     every output the header lets be NULL is NULL (obj_by_k, status, x, c; the evaluation's cycle,
           bottleneck, reason, x, c).
Every output array starts from the same sentinel on both sides and is compared whole, except the dense x / c:
an instance of a fleet of M < max_devices devices owns 7 max_devices + 1 entries of which the kernels write
the first 7 M + 1 only (what the staging buffer held before is what a host entry returns in the rest), so
the dense comparison is over those 7 M + 1 entries of every instance. Everything is exact: no tolerance.

halda_solve_fleets_host has three transports; the table is run through all of them -- the default context
(zero-copy through the mapped pinned buffer) and a second context created under HALDA_HOST_PATH=copy, each
with ordinary NumPy arrays (staged through the pinned buffer on the second context) and with every array in
halda_host_alloc blocks (direct DMA on the second context). Which route a call took is not asserted."""

import ctypes
import os
from functools import lru_cache

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import subfleets as sf
from distilp_amd.solver import variants as va
from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaBoxC, HaldaFleetResultC, HaldaPlanResultC,
                                       HaldaPlansC, _fleets_struct, _host_arrays,
                                       fleet_table, model_struct)
from distilp_amd.synth import synth_fleet

from .helpers import synth_devices

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5)
KS = (4, 20, 40)
ITEMS = ((0, (1, 0)), (1, (2, 0)), (2, (4, 1, 3)), (2, (0, 1, 2, 3, 4)), (1, (1,)))  # ragged: the expansion route
LAYOUTS = ("dense", "compact", "bare")
TABLE_FIELDS = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
SWEEP_OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c")
EVAL_OUTS = ("status", "obj_value", "cycle", "bottleneck", "reason", "x", "c")
I32 = ("best_k", "w", "n", "status", "bottleneck", "reason")
SENTINEL = -7


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


_SHARED = {}  # the table and the device entries' results, computed once


def _table(model):
    if "table" not in _SHARED:
        fleets = [synth_devices(M, 700 + M, synth_fleet(700 + M, M)) for M in SIZES]
        _SHARED["table"] = fleet_table(fleets, model)
    return _SHARED["table"]


def _lib(ctx):
    return ctx.lib


@lru_cache(maxsize=None)
def _copy_context():
    """A second context whose halda_solve_fleets_host never takes the zero-copy route."""
    old = os.environ.get("HALDA_HOST_PATH")
    os.environ["HALDA_HOST_PATH"] = "copy"
    try:
        return lh.HaldaContext(0)
    finally:
        if old is None:
            os.environ.pop("HALDA_HOST_PATH", None)
        else:
            os.environ["HALDA_HOST_PATH"] = old


def _host_fleets(table, alloc=np.empty):
    arrs = {}
    for f in TABLE_FIELDS:
        src = np.ascontiguousarray(getattr(table, f))
        arrs[f] = alloc(src.shape, src.dtype)
        arrs[f][...] = src
    return arrs, _fleets_struct(table, lambda f: arrs[f].ctypes.data)


def _pinned(shape, dtype):
    return _host_arrays(((shape, dtype),))[0]


def _device_fleets(table):
    torch, dev = _torch()
    arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in TABLE_FIELDS}
    return arrs, _fleets_struct(table, lambda f: arrs[f].data_ptr())


class Outs:
    """Sentinel-filled output arrays of `names` over `rows` fleets (or items, or variant x fleet) of `lens`
    devices and `per` instances each, in one layout; .mask selects the entries of x / c that are compared."""

    def __init__(self, names, lens, per, n_dev, layout, max_devices):
        lens = np.asarray(lens, np.int64)
        rows, inst = len(lens), len(lens) * per
        need = np.repeat(7 * lens + 1, per)
        self.x_off, self.mask = None, slice(None)
        if layout == "compact":
            keep = np.ones(inst, bool)
            keep[1] = False  # one instance whose x / c are not wanted
            off = np.cumsum(np.where(keep, need, 0)) - np.where(keep, need, 0)
            self.x_off = np.where(keep, off, -1).astype(np.int64)
            xlen = int(np.where(keep, need, 0).sum())
        else:
            stride = 7 * max_devices + 1
            xlen = inst * stride
            self.mask = (np.arange(stride)[None, :] < need[:, None]).ravel()
        size = {"best_k": rows, "obj_value": rows, "w": n_dev, "n": n_dev, "obj_by_k": inst, "status": inst,
                "cycle": rows, "bottleneck": rows, "reason": rows, "x": xlen, "c": xlen}
        optional = set(names) - {"best_k", "obj_value", "w", "n"} - ({"status"} if "cycle" in names else set())
        self.names = [f for f in names if not (layout == "bare" and f in optional)]
        self.a = {f: np.full(size[f], SENTINEL, np.int32 if f in I32 else np.float64) for f in self.names}
        self.all_names = names

    def struct(self, cls, ptr, x_off_ptr):
        return cls(*[ptr(f) if f in self.a else None for f in self.all_names],
                   x_off_ptr if self.x_off is not None and "x" in self.a else None)

    def host(self, cls, alloc=None):
        if alloc is not None:
            for f, src in list(self.a.items()):
                self.a[f] = alloc(src.shape, src.dtype)
                self.a[f][...] = src
            if self.x_off is not None:
                src, self.x_off = self.x_off, alloc(self.x_off.shape, np.int64)
                self.x_off[...] = src
        return self.struct(cls, lambda f: self.a[f].ctypes.data, None if self.x_off is None else self.x_off.ctypes.data)

    def device(self, cls):
        torch, dev = _torch()
        self.t = {f: torch.from_numpy(v).to(dev) for f, v in self.a.items()}
        self.t_off = None if self.x_off is None else torch.from_numpy(self.x_off).to(dev)
        return self.struct(cls, lambda f: self.t[f].data_ptr(), None if self.t_off is None else self.t_off.data_ptr())

    def fetch(self):
        torch, dev = _torch()
        torch.cuda.synchronize(dev)
        self.a = {f: t.cpu().numpy() for f, t in self.t.items()}
        return self


def _same(got, want, what):
    assert got.names == want.names
    for f in got.names:
        g, w = got.a[f], want.a[f]
        if f in ("x", "c"):
            g, w = g[got.mask], w[want.mask]
        assert g.tobytes() == w.tobytes(), (what, f)
        assert not (f not in ("x", "c") and (g == SENTINEL).any()), (what, f, "an entry was never written")


def _sweep_outs(table, layout, lens=None, per=len(KS), n_dev=None):
    lens = table.sizes() if lens is None else lens
    return Outs(SWEEP_OUTS, lens, per, table.n_devices if n_dev is None else n_dev, layout, int(max(lens)))


def _call(lib, fn, *args):
    rc = getattr(lib, fn)(*args)
    assert rc == 0, (fn, rc, lh.last_error(lib))


def _karr():
    return np.asarray(KS, np.int32)


def _model(model, kv=0.5):
    return model_struct(model, kv)


# ---------------------------------------------------------------- halda_solve_fleets_host: three transports
def _fleets_device(model, layout):
    if layout not in _SHARED:
        _SHARED[layout] = _fleets_device_run(model, layout)
    return _SHARED[layout]


def _fleets_device_run(model, layout):
    table, ctx = _table(model), lh.get_context(0)
    lib, k = _lib(ctx), _karr()
    arrs, fs = _device_fleets(table)
    o = _sweep_outs(table, layout)
    r = o.device(HaldaFleetResultC)
    with ctx._lock:
        _call(lib, "halda_solve_fleets", ctx.ctx, ctypes.byref(_model(model)), ctypes.byref(fs), k.ctypes.data,
              len(KS), ctypes.byref(r), None)
    return o.fetch()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pinned", [False, True], ids=["numpy", "host_alloc"])
@pytest.mark.parametrize("copy_ctx", [False, True], ids=["default_ctx", "copy_ctx"])
def test_fleets_host_equals_device_entry_on_every_transport(llama_online_model, copy_ctx, pinned, layout):
    model, table = llama_online_model, _table(llama_online_model)
    ctx = _copy_context() if copy_ctx else lh.get_context(0)
    lib, k = _lib(ctx), _karr()
    alloc = _pinned if pinned else None
    if pinned:
        kp = _pinned(k.shape, np.int32)
        kp[...] = k
        k = kp
    arrs, fs = _host_fleets(table, alloc or np.empty)
    o = _sweep_outs(table, layout)
    r = o.host(HaldaFleetResultC, alloc)
    with ctx._lock:
        _call(lib, "halda_solve_fleets_host", ctx.ctx, ctypes.byref(_model(model)), ctypes.byref(fs), k.ctypes.data,
              len(KS), ctypes.byref(r))
    _same(o, _fleets_device(model, layout), "halda_solve_fleets_host")
    if layout != "bare":  # the table does what the docstring says: k = 20 and k = 40 leave fleets infeasible
        st = o.a["status"].reshape(len(SIZES), len(KS))
        assert st[2, 1] == lh.STATUS_INFEASIBLE and (st[1:, 2] == lh.STATUS_INFEASIBLE).all()
        assert (st == lh.STATUS_OPTIMAL).any()


# ---------------------------------------------------------------- sub-fleets
def _items(table, make):
    parent, sub_off, sub_idx = sf.pack_items(table.sizes(), [(p, list(s)) for p, s in ITEMS])
    lens = np.diff(sub_off)
    keep = [make(a) for a in (parent, sub_off, sub_idx)]
    return keep, lens


@pytest.mark.parametrize("layout", LAYOUTS)
def test_subfleets_host_equals_device_entry(llama_online_model, layout):
    torch, dev = _torch()
    model, table, ctx = llama_online_model, _table(llama_online_model), lh.get_context(0)
    lib, k, m = _lib(ctx), _karr(), _model(llama_online_model)
    keep_h, lens = _items(table, np.ascontiguousarray)
    tot = int(lens.sum())
    arrs, fs = _host_fleets(table)
    got = _sweep_outs(table, layout, lens, n_dev=tot)
    it = sf.HaldaSubfleetsC(len(lens), int(lens.min()), int(lens.max()), *[a.ctypes.data for a in keep_h])
    r = got.host(HaldaFleetResultC)
    with ctx._lock:
        _call(lib, "halda_solve_subfleets_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
              k.ctypes.data, len(KS), ctypes.byref(r))
    keep_d, _ = _items(table, lambda a: torch.from_numpy(a).to(dev))
    darrs, dfs = _device_fleets(table)
    want = _sweep_outs(table, layout, lens, n_dev=tot)
    it = sf.HaldaSubfleetsC(len(lens), int(lens.min()), int(lens.max()), *[t.data_ptr() for t in keep_d])
    r = want.device(HaldaFleetResultC)
    with ctx._lock:
        _call(lib, "halda_solve_subfleets", ctx.ctx, ctypes.byref(m), ctypes.byref(dfs), ctypes.byref(it),
              k.ctypes.data, len(KS), ctypes.byref(r), None)
    _same(got, want.fetch(), "halda_solve_subfleets_host")


# ---------------------------------------------------------------- two model variants
@pytest.mark.parametrize("layout", LAYOUTS)
def test_variants_host_equals_device_entry(llama_online_model, layout):
    model, table, ctx = llama_online_model, _table(llama_online_model), lh.get_context(0)
    lib, k = _lib(ctx), _karr()
    nv = 2
    models = (type(_model(model)) * nv)(_model(model, 0.5), _model(model, 1.0))
    lens = np.tile(table.sizes(), nv)

    def outs():
        return _sweep_outs(table, layout, lens, n_dev=nv * table.n_devices)

    arrs, fs = _host_fleets(table)
    got = outs()
    r = got.host(HaldaFleetResultC)
    with ctx._lock:
        _call(lib, "halda_solve_variants_host", ctx.ctx, models, nv, ctypes.byref(fs), k.ctypes.data, len(KS),
              ctypes.byref(r))
    darrs, dfs = _device_fleets(table)
    want = outs()
    r = want.device(HaldaFleetResultC)
    with ctx._lock:
        _call(lib, "halda_solve_variants", ctx.ctx, models, nv, ctypes.byref(dfs), k.ctypes.data, len(KS),
              ctypes.byref(r), None)
    _same(got, want.fetch(), "halda_solve_variants_host")


# ---------------------------------------------------------------- plans: the evaluation alone, and with the sweep
def _plans(table, model, make):
    """The table's own best plan per fleet (the default-layout sweep's best_k / w / n), one w moved."""
    best = _fleets_device(model, "dense").a
    w = best["w"].copy()
    w[0] += 1  # fleet 0's plan no longer sums to W: an infeasible plan among feasible ones
    keep = [make(np.ascontiguousarray(a)) for a in (best["best_k"].copy(), w, best["n"].copy())]
    return keep


def _eval_outs(table, layout):
    return Outs(EVAL_OUTS, table.sizes(), 1, table.n_devices, layout, int(table.sizes().max()))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sweep", [False, True], ids=["halda_eval_plans_host", "halda_solve_fleets_plans_host"])
def test_plans_host_equals_device_entry(llama_online_model, sweep, layout):
    torch, dev = _torch()
    model, table, ctx = llama_online_model, _table(llama_online_model), lh.get_context(0)
    lib, k, m = _lib(ctx), _karr(), _model(llama_online_model)
    both = []
    for side in ("host", "device"):
        host = side == "host"
        arrs, fs = _host_fleets(table) if host else _device_fleets(table)
        keep = _plans(table, model, (lambda a: a) if host else (lambda a: torch.from_numpy(a).to(dev)))
        p = HaldaPlansC(*[a.ctypes.data if host else a.data_ptr() for a in keep])
        e, o = _eval_outs(table, layout), _sweep_outs(table, layout)
        er = e.host(HaldaPlanResultC) if host else e.device(HaldaPlanResultC)
        sr = o.host(HaldaFleetResultC) if host else o.device(HaldaFleetResultC)
        tail = () if host else (None,)
        with ctx._lock:
            if sweep:
                _call(lib, "halda_solve_fleets_plans" + ("_host" if host else ""), ctx.ctx, ctypes.byref(m),
                      ctypes.byref(fs), k.ctypes.data, len(KS), ctypes.byref(p), ctypes.byref(er), ctypes.byref(sr),
                      *tail)
            else:
                _call(lib, "halda_eval_plans" + ("_host" if host else ""), ctx.ctx, ctypes.byref(m),
                      ctypes.byref(fs), ctypes.byref(p), ctypes.byref(er), *tail)
        both.append((e, o) if host else (e.fetch(), o.fetch()))
    (ge, go), (we, wo) = both
    _same(ge, we, "the evaluation")
    if sweep:
        _same(go, wo, "the sweep")
    solved = _fleets_device(model, "dense").a["best_k"] > 0
    assert ge.a["status"][0] == lh.STATUS_INFEASIBLE and (ge.a["status"][1:][solved[1:]] == lh.STATUS_OPTIMAL).all()


# ---------------------------------------------------------------- the boxed sweep
@pytest.mark.parametrize("layout", LAYOUTS)
def test_boxed_host_equals_device_entry(llama_online_model, layout):
    torch, dev = _torch()
    model, table, ctx = llama_online_model, _table(llama_online_model), lh.get_context(0)
    lib, k, m = _lib(ctx), _karr(), _model(llama_online_model)
    nd = table.n_devices
    w_max = np.full(nd, np.iinfo(np.int32).max, np.int32)
    w_max[3] = 1  # a cap on one device of the 3-device fleet
    n_min = np.zeros(nd, np.int32)
    n_max = np.full(nd, np.iinfo(np.int32).max, np.int32)
    n_max[5] = 0  # one device of the 5-device fleet keeps its GPU idle
    box = (None, w_max, n_min, n_max)  # w_min absent: an optional input array that is skipped
    arrs, fs = _host_fleets(table)
    got = _sweep_outs(table, layout)
    r = got.host(HaldaFleetResultC)
    b = HaldaBoxC(*[None if a is None else a.ctypes.data for a in box])
    with ctx._lock:
        _call(lib, "halda_solve_fleets_boxed_host", ctx.ctx, ctypes.byref(m), ctypes.byref(fs), k.ctypes.data,
              len(KS), ctypes.byref(b), ctypes.byref(r))
    darrs, dfs = _device_fleets(table)
    dbox = [None if a is None else torch.from_numpy(a).to(dev) for a in box]
    want = _sweep_outs(table, layout)
    r = want.device(HaldaFleetResultC)
    b = HaldaBoxC(*[None if t is None else t.data_ptr() for t in dbox])
    with ctx._lock:
        _call(lib, "halda_solve_fleets_boxed", ctx.ctx, ctypes.byref(m), ctypes.byref(dfs), k.ctypes.data, len(KS),
              ctypes.byref(b), ctypes.byref(r), None)
    _same(got, want.fetch(), "halda_solve_fleets_boxed_host")
