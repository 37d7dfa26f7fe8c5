"""Model variants of one fleet table on the GPU (libhalda halda_solve_variants): slice v of every output
equals, bit for bit, what halda_solve_fleets writes for models[v] -- through the fused register route
(halda_sweep_variants_kernel), the fused table route (halda_sweep_tables_variants_kernel), the per-variant
loop, and the Python entries built on them -- and the reference's recorded grid (tests/golden/variants.json).
The route is asserted in every case: a fused kernel is compared only where it really ran."""

import contextlib
import ctypes
import io

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import halda_context_sweep, halda_solve_batch, halda_solve_variants, model_grid
from distilp_amd.solver import variants as va
from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaFleetResultC, _fleets_struct, fleet_table,
                                       open_x_offsets)
from distilp_amd.synth import synth_fleet

from .conftest import REPO, load_json
from .helpers import fixture_fleet, synth_devices

pytestmark = pytest.mark.gpu

KS80 = [1, 2, 4, 5, 8, 10, 16, 20, 40]  # the default k list of the 80-layer model
OUTS = ("best_k", "obj_value", "w", "n", "obj_by_k", "status", "x", "c")
TABLE_FIELDS = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
GUARD = 3  # entries of -7 behind every array: nothing outside the n_var slices is written


def fleet(M, seed):
    return synth_devices(M, seed, synth_fleet(seed, M))


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _upload(table):
    torch, dev = _torch()
    arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in TABLE_FIELDS}
    return arrs, _fleets_struct(table, lambda f: arrs[f].data_ptr())


def _results(n, tot, ninst, xlen, x_off=None, want=OUTS):
    """Device result arrays pre-filled with -7 (x / c with zeros: the dense layout's tail past 7 M + 1 is
    never written), GUARD more entries behind each."""
    torch, dev = _torch()

    def full(k, v, dt):
        return torch.full((k + GUARD,), v, dtype=dt, device=dev)

    o = {"best_k": full(n, -7, torch.int32), "obj_value": full(n, -7.0, torch.float64),
         "w": full(tot, -7, torch.int32), "n": full(tot, -7, torch.int32),
         "obj_by_k": full(ninst, -7.0, torch.float64), "status": full(ninst, -7, torch.int32),
         "x": torch.zeros(xlen + GUARD, dtype=torch.float64, device=dev),
         "c": torch.zeros(xlen + GUARD, dtype=torch.float64, device=dev)}
    o["x"][xlen:] = -7.0
    o["c"][xlen:] = -7.0
    xo = None if x_off is None else torch.from_numpy(np.ascontiguousarray(x_off)).to(dev)
    r = HaldaFleetResultC(*[o[f].data_ptr() if f in want else None for f in OUTS],
                          xo.data_ptr() if xo is not None else None)
    return o, r, xo


def _collect(o, want=OUTS):
    out = {}
    for f in OUTS:
        a = o[f].cpu().numpy()
        assert (a[-GUARD:] == -7).all(), f  # the guard behind the array
        out[f] = a[:-GUARD]
        if f not in want:
            assert (out[f] == (0 if f in ("x", "c") else -7)).all(), f  # an output not asked for is not written
    return out


def _xlen(sizes, nk, x_off, n_var=1):
    if x_off is None:
        return n_var * len(sizes) * nk * (7 * int(sizes.max()) + 1)
    return int(np.max(x_off + np.tile(np.repeat(7 * sizes + 1, nk), n_var), initial=0))


def solve_fleets_device(table, mstruct, ks, x_off=None, want=OUTS):
    """halda_solve_fleets on a device copy of `table` for one halda_model: every output, as NumPy arrays."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    lib = ctx.lib
    arrs, fs = _upload(table)
    sizes, nk, nf = table.sizes(), len(ks), table.n_fleets
    o, r, xo = _results(nf, table.n_devices, nf * nk, _xlen(sizes, nk, x_off), x_off, want)
    karr = np.asarray(ks, np.int32)
    with ctx._lock:
        rc = lib.halda_solve_fleets(ctx.ctx, ctypes.byref(mstruct), ctypes.byref(fs), karr.ctypes.data, nk,
                                    ctypes.byref(r), None)
    assert rc == 0, lh.last_error(lib)
    torch.cuda.synchronize(dev)
    return _collect(o, want)


def solve_variants_device(table, variants, ks, path=0, x_off=None, want=OUTS, stream=None):
    """halda_solve_variants on a device copy of `table`: every output (variant-major) and the route."""
    torch, dev = _torch()
    ctx = lh.get_context(0)
    lib = ctx.lib
    arrs, fs = _upload(table)
    sizes, nk, nf, nd, nv = table.sizes(), len(ks), table.n_fleets, table.n_devices, len(variants)
    o, r, xo = _results(nv * nf, nv * nd, nv * nf * nk, _xlen(sizes, nk, x_off, nv), x_off, want)
    karr = np.asarray(ks, np.int32)
    ms = va.model_structs(variants)
    torch.cuda.synchronize(dev)
    va.set_variants_path(ctx, path)
    try:
        with ctx._lock:
            rc = lib.halda_solve_variants(ctx.ctx, ms, nv, ctypes.byref(fs), karr.ctypes.data, nk, ctypes.byref(r),
                                          ctypes.c_void_p(stream.cuda_stream) if stream is not None else None)
    finally:
        va.set_variants_path(ctx, 0)
    assert rc == 0, lh.last_error(lib)
    torch.cuda.synchronize(dev)
    return dict(_collect(o, want), route=va.last_variants_route(ctx))


def variant_slices(got, table, nk, nv, x_off1=None):
    """The variant-major outputs cut into one dict per variant, each shaped like halda_solve_fleets' own."""
    nf, nd = table.n_fleets, table.n_devices
    o = va.variant_offsets(nv, nf, nd, nk)
    xs = 7 * int(table.sizes().max()) + 1
    ext = None if x_off1 is None else _xlen(table.sizes(), nk, x_off1)
    out = []
    for v in range(nv):
        d = {}
        for f, n in (("best_k", nf), ("obj_value", nf), ("w", nd), ("n", nd), ("obj_by_k", nf * nk),
                     ("status", nf * nk)):
            a = int(o[f][v])
            d[f] = got[f][a:a + n]
        for f in ("x", "c"):
            d[f] = got[f][v * nf * nk * xs:(v + 1) * nf * nk * xs] if ext is None else got[f][v * ext:(v + 1) * ext]
        out.append(d)
    return out


def assert_same_bits(got, want, what):
    for f in OUTS:
        a, b = got[f], want[f]
        assert a.shape == b.shape and np.array_equal(a, b) and a.tobytes() == b.tobytes(), (
            what, f, np.flatnonzero(a != b)[:8])


def check_variants(fleets, variants, ks=KS80, paths=((0, "fused"),), compact=False, want=OUTS):
    """Every output of halda_solve_variants on each (path, expected route) against len(variants) separate
    halda_solve_fleets calls. Returns the per-variant reference outputs."""
    table = fleet_table(fleets, variants[0][0])
    nk, nv = len(ks), len(variants)
    x1 = open_x_offsets(table, variants[0][0], ks) if compact else None
    xv = None if x1 is None else va.variant_x_offsets(x1, _xlen(table.sizes(), nk, x1), nv)
    ms = va.model_structs(variants)
    wants = [solve_fleets_device(table, ms[v], ks, x1, want) for v in range(nv)]
    for w in wants:
        assert not (w["best_k"] == -7).any() and not (w["w"] == -7).any()
    for path, route in paths:
        got = solve_variants_device(table, variants, ks, path, xv, want)
        assert got["route"] == route, (path, got["route"])
        for v, sl in enumerate(variant_slices(got, table, nk, nv, x1)):
            assert_same_bits(sl, wants[v], f"path {path} variant {v}")
    return wants


# ---------------------------------------------------------------- the routes
def test_register_route_fused_and_looped(llama_online_model):
    """5 fleets (not a multiple of the 4 waves per workgroup) of 64 devices x 3 variants: the register sweep
    alone, one wave per (variant, fleet); and the same call on path 1."""
    fleets = [fleet(64, 5100 + i) for i in range(5)]
    variants = [(llama_online_model, "4bit"), (llama_online_model.model_copy(update={"n_kv": 65536}), "fp16"),
                (llama_online_model.model_copy(update={"n_kv": 1 << 18}), "8bit")]
    wants = check_variants(fleets, variants, paths=((0, "fused"), (1, "loop")))
    assert all((w["best_k"] > 0).any() for w in wants)
    assert wants[0]["obj_value"].tobytes() != wants[1]["obj_value"].tobytes()


def test_register_route_compact_x(llama_online_model):
    fleets = [fleet(64, 5100 + i) for i in range(5)]
    check_variants(fleets, model_grid(llama_online_model, ("4bit", "fp16"), [512, 65536])[:3], compact=True,
                   paths=((0, "fused"), (1, "loop")))


def test_table_route_one_fixture_fleet_five_variants(llama_online_model):
    devs = synth_devices(4, 0)  # a 4-device fleet of the recorded synthetic fixtures
    variants = model_grid(llama_online_model, ("4bit", "8bit", "fp16"), [512, 1 << 20])[:5]
    wants = check_variants([devs], variants, paths=((0, "fused"), (1, "loop")))
    assert len({w["obj_value"].tobytes() for w in wants}) >= 4
    assert all((w["status"] == lh.STATUS_OPTIMAL).sum() >= 2 for w in wants)  # k > 1 tables ran


@pytest.mark.parametrize("compact", [False, True])
def test_table_route_mixed_sizes(llama_online_model, compact):
    fleets = [fleet(2, 5201), fleet(3, 5202), fleet(5, 5203)]
    variants = [(llama_online_model, "8bit"), (llama_online_model.model_copy(update={"n_kv": 1 << 18}), "fp16"),
                (llama_online_model.model_copy(update={"n_kv": 1 << 20}), "4bit")]
    check_variants(fleets, variants, compact=compact, paths=((0, "fused"), (1, "loop")))


def test_table_route_without_per_k_outputs(llama_online_model):
    fleets = [fleet(2, 5201), fleet(3, 5202), fleet(5, 5203)]
    variants = model_grid(llama_online_model, ("4bit", "fp16"), [512, 1 << 19])[:3]
    check_variants(fleets, variants, want=("best_k", "obj_value", "w", "n"), paths=((0, "fused"), (1, "loop")))
    check_variants([fleet(64, 5100 + i) for i in range(5)], variants, want=("best_k", "obj_value", "w", "n"))


def test_kslot_shape_takes_the_loop(llama_online_model):
    """70 fleets of 3..16 devices plan as the k-slot sweep with a gated table launch: route 2, equal results."""
    fleets = [fleet(3 + i % 14, 5300 + i) for i in range(70)]
    variants = [(llama_online_model, "4bit"), (llama_online_model.model_copy(update={"n_kv": 65536}), "fp16")]
    check_variants(fleets, variants, paths=((0, "loop"),))


@pytest.mark.parametrize("shape", ["register", "tables"])
def test_the_whole_model_is_per_variant(llama_online_model, shape):
    """Variants that differ from the base in ONE model field (b_in, b_out, V, b_layer, f_q["b_1"]) at the same
    n_kv and kv_bits: each slice differs from the base slice and equals its own single call."""
    m = llama_online_model
    fleets = [fleet(64, 5100 + i) for i in range(5)] if shape == "register" else [fleet(2, 5201), fleet(3, 5202),
                                                                               fleet(5, 5203)]
    edits = [{"b_in": m.b_in * 3}, {"b_out": m.b_out * 5}, {"V": m.V * 2}, {"b_layer": int(m.b_layer * 1.5)},
             {"f_q": dict(m.f_q, b_1=m.f_q["b_1"] * 3)}]
    variants = [(m, "8bit")] + [(m.model_copy(update=u), "8bit") for u in edits]
    ms = va.model_structs(variants)
    # b_prime is not what differs (b_layer enters it: dense_common.py:25-46)
    assert len({ms[v].b_prime for v in range(len(variants)) if v != 4}) == 1
    wants = check_variants(fleets, variants)
    for v in range(1, len(variants)):
        assert any(wants[v][f].tobytes() != wants[0][f].tobytes() for f in OUTS), edits[v - 1]


@pytest.mark.parametrize("shape", ["register", "tables"])
def test_one_variant_equals_halda_solve_fleets(llama_online_model, shape):
    fleets = [fleet(64, 5100)] if shape == "register" else [synth_devices(4, 1)]
    check_variants(fleets, [(llama_online_model, "fp16")], paths=((0, "fused"), (1, "loop")))


def test_on_a_callers_stream(llama_online_model):
    torch, dev = _torch()
    fleets = [fleet(64, 5100 + i) for i in range(5)]
    variants = model_grid(llama_online_model, ("4bit", "fp16"), [512, 65536])
    table = fleet_table(fleets, llama_online_model)
    a = solve_variants_device(table, variants, KS80)
    b = solve_variants_device(table, variants, KS80, stream=torch.cuda.Stream(dev))
    assert a["route"] == b["route"] == "fused"
    assert_same_bits(a, b, "stream")


# ---------------------------------------------------------------- argument errors
def test_argument_errors_launch_nothing(llama_online_model):
    torch, dev = _torch()
    ctx = lh.get_context(0)
    lib = ctx.lib
    m = llama_online_model
    table = fleet_table([fleet(64, 5100)], m)
    arrs, fs = _upload(table)
    nk = len(KS80)
    karr = np.asarray(KS80, np.int32)
    good = va.model_structs([(m, "8bit"), (m, "4bit")])
    check_variants([fleet(64, 5100)], [(m, "8bit")])  # a good call first: the route it leaves is "fused"
    mixed_L = va.model_structs([(m, "8bit"), (m.model_copy(update={"L": 40}), "8bit")])
    mixed_fq = va.model_structs([(m, "8bit"), (m, "8bit")])
    mixed_fq[1].has_f_q = 0
    for ms, nv, msg in ((mixed_L, 2, "L = 40"), (mixed_fq, 2, "has_f_q"), (good, 0, "n_var"), (good, 65536, "n_var")):
        o, r, _ = _results(2, 2 * 64, 2 * nk, 2 * nk * (7 * 64 + 1))
        with ctx._lock:
            rc = lib.halda_solve_variants(ctx.ctx, ms, nv, ctypes.byref(fs), karr.ctypes.data, nk, ctypes.byref(r), None)
            err = lh.last_error(lib)
            rch = lib.halda_solve_variants_host(ctx.ctx, ms, nv, ctypes.byref(fs), karr.ctypes.data, nk,
                                                ctypes.byref(r))
        assert rc == -22 and rch == -22 and msg in err and msg in lh.last_error(lib), (rc, rch, err)
        torch.cuda.synchronize(dev)
        got = _collect(o)
        for f in OUTS:
            assert (got[f] == (0 if f in ("x", "c") else -7)).all(), f  # nothing was launched
    assert va.last_variants_route(ctx) == "fused"
    with pytest.raises(RuntimeError, match="variants path"):
        va.set_variants_path(ctx, 2)


# ---------------------------------------------------------------- the Python entries
def same_results(a, b):
    if a is None or b is None:
        return a is None and b is None
    return (a.k, a.w, a.n, a.sets) == (b.k, b.w, b.n, b.sets) and \
        np.float64(a.obj_value).tobytes() == np.float64(b.obj_value).tobytes()


def test_python_entry_equals_halda_solve_batch_per_variant(llama_online_model):
    m = llama_online_model
    fleets = [fleet(2, 5201), fleet(3, 5202), fleet(5, 5203), fleet(64, 5100), fleet(100, 5400)]
    variants = model_grid(m, ("4bit", "8bit", "fp16"), [512, 1 << 18, 1 << 21])
    variants.append((m.model_copy(update={"b_in": m.b_in * 3, "V": m.V * 2}), "8bit"))
    got = halda_solve_variants(fleets, variants)
    assert len(got) == len(variants)
    seen = set()
    for (mv, kv), row in zip(variants, got):
        want = halda_solve_batch(fleets, mv, kv_bits=kv)
        assert len(row) == len(want) == len(fleets)
        for f, (a, b) in enumerate(zip(row, want)):
            assert same_results(a, b), (mv.n_kv, kv, f, a, b)
        seen.add(tuple(None if r is None else (r.k, tuple(r.w)) for r in row))
        assert row[4] is None  # 100 devices over 80 layers: no k is feasible
    assert len(seen) >= 3  # the variants change the plans
    # a k list of the caller's, and one fleet through halda_context_sweep
    ks = [2, 1, 4]
    got = halda_solve_variants(fleets[:3], variants[:4], k_candidates=ks)
    for (mv, kv), row in zip(variants[:4], got):
        assert all(same_results(a, b) for a, b in zip(row, halda_solve_batch(fleets[:3], mv, ks, kv_bits=kv)))
    rows = halda_context_sweep(fleets[1], m, [512, 1 << 20], ("4bit", "fp16"))
    assert [(n, kv) for n, kv, _ in rows] == [(512, "4bit"), (512, "fp16"), (1 << 20, "4bit"), (1 << 20, "fp16")]
    for n, kv, r in rows:
        assert same_results(r, halda_solve_batch([fleets[1]], m.model_copy(update={"n_kv": n}), kv_bits=kv)[0])


def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


@pytest.mark.parametrize("folder", ["llama_3_70b/online", "hermes_70b"])
def test_python_entry_equals_the_reference_grid(folder):
    g = load_json("variants.json")
    cases = g["folders"][folder]
    devs, model = fixture_fleet(folder)
    rows = halda_context_sweep(devs, model, g["n_kv"], tuple(g["kv_bits"]), mip_gap=g["mip_gap"])
    assert len(rows) == len(cases) == 12
    for (n, kv, r), c in zip(rows, cases):
        ref = c["result"]
        assert (n, kv) == (c["n_kv"], c["kv_bits"])
        assert (r.k, r.w, r.n, r.sets) == (ref["k"], ref["w"], ref["n"], ref["sets"]), (n, kv, r, ref)
        assert close(r.obj_value, ref["obj_value"]), (n, kv, r.obj_value, ref["obj_value"])


def test_cli_lines(monkeypatch):
    from distilp_amd.cli.solver import main

    monkeypatch.chdir(REPO)
    g = load_json("variants.json")

    def run(argv):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert main(argv) == 0
        return buf.getvalue()

    base = ["--profile", "llama_3_70b/online", "--quiet", "--no-plot"]
    plain = run(base)
    both = run(base + ["--kv-sweep", "4bit", "8bit", "fp16", "--n-kv-sweep"] + [str(n) for n in g["n_kv"]])
    assert both.startswith(plain)  # the output without the flags, byte for byte, then the grid
    lines = both[len(plain):].splitlines()
    cases = g["folders"]["llama_3_70b/online"]
    assert len(lines) == len(cases)
    for line, c in zip(lines, cases):
        head, _, tail = line.partition(": ")
        assert head == f"n_kv={c['n_kv']}, kv_bits={c['kv_bits']}"
        k, obj = tail.split(", ")
        assert k == f"k={c['result']['k']}" and close(float(obj[len("obj="):]), round(c["result"]["obj_value"], 6))
    # either flag alone sweeps its axis at the model's other value (n_kv 512; the solve's own 4bit)
    kv_only = run(base + ["--kv-sweep", "8bit", "fp16"])[len(plain):].splitlines()
    assert [ln.partition(": ")[0] for ln in kv_only] == ["n_kv=512, kv_bits=8bit", "n_kv=512, kv_bits=fp16"]
    n_only = run(base + ["--n-kv-sweep", "65536"])[len(plain):].splitlines()
    assert [ln.partition(": ")[0] for ln in n_only] == ["n_kv=65536, kv_bits=4bit"]
    assert n_only[0].endswith(f"k={cases[3]['result']['k']}, obj={cases[3]['result']['obj_value']:.6f}")
