"""Model variants of one fleet table (distilp_amd/solver/variants.py), host side: the grid, the argument
errors, the variant-major offsets against a NumPy restatement, the per-variant constants against a table
packed for that variant, the CLI flags, the new kernels' code objects, and the oracle pinned to the
reference's recorded results (tests/golden/variants.json). No GPU."""

import ctypes

import numpy as np
import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import variants as va
from distilp_amd.solver.fleets import fleet_constants, fleet_table, open_x_offsets
from oracle import milp_oracle as mo

from .conftest import load_json
from .helpers import fixture_fleet, synth_devices
from .test_abi import kernel_resources

NAMES = ("halda_solve_variants", "halda_solve_variants_host", "halda_set_variants_path", "halda_last_variants_route")


def test_new_entry_points_are_exported_and_reject_bad_arguments():
    for name in NAMES:
        assert name in lh.EXPORTS
    raw = ctypes.CDLL(str(lh.LIB_PATH))
    lib = lh.load_library()
    raw.halda_set_variants_path.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert raw.halda_set_variants_path(None, 0) == -22
    raw.halda_last_variants_route.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert raw.halda_last_variants_route(None, None) == -22
    raw.halda_solve_variants_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert raw.halda_solve_variants_host(None, None, 1, None, None, 1, None) == -22
    assert "NULL" in lh.last_error(lib)
    import distilp.solver
    import distilp_amd.solver

    for mod in (distilp.solver, distilp_amd.solver):
        for name in ("halda_solve_variants", "halda_context_sweep", "model_grid"):
            assert getattr(mod, name) is getattr(va, name)


def test_model_grid_order_and_contents(llama_online_model):
    m = llama_online_model
    g = va.model_grid(m, ("4bit", "fp16"), [512, 4096, 64])
    assert [(x.n_kv, kv) for x, kv in g] == [(512, "4bit"), (512, "fp16"), (4096, "4bit"), (4096, "fp16"),
                                               (64, "4bit"), (64, "fp16")]  # n_kv outermost, in the given order
    for x, _ in g:
        assert x is not m and x.model_copy(update={"n_kv": m.n_kv}) == m  # nothing but n_kv differs
    assert [(x.n_kv, kv) for x, kv in va.model_grid(m)] == [(m.n_kv, "8bit")]
    assert [(x.n_kv, kv) for x, kv in va.model_grid(m, "fp16")] == [(m.n_kv, "fp16")]
    assert [(x.n_kv, kv) for x, kv in va.model_grid(m, n_kv=(n for n in (1, 2)))] == [(1, "8bit"), (2, "8bit")]


def test_variants_that_cannot_share_a_table_raise(llama_online_model):
    m = llama_online_model
    devs = synth_devices(4, 0)
    no_fq = {k: v for k, v in m.f_q.items() if k != "b_1"}
    no_fout = {k: v for k, v in m.f_out.items() if k != "b_1"}
    for update, what in (({"L": m.L + 1}, "L = 81"), ({"Q": "F16" if m.Q != "F16" else "Q8_0"}, "Q = "),
                         ({"f_q": no_fq}, "in f_q"), ({"f_out": no_fout}, "in f_out")):
        other = m.model_copy(update=update)
        with pytest.raises(ValueError, match=what):
            va.halda_solve_variants([devs], [(m, "8bit"), (m, "4bit"), (other, "8bit")])  # before any GPU call
    with pytest.raises(ValueError, match="Unsupported kv_bits"):
        va.halda_solve_variants([devs], [(m, "8bit"), (m, "3bit")])
    assert va.halda_solve_variants([devs], []) == []
    assert va.halda_solve_variants([], [(m, "8bit"), (m, "4bit")]) == [[], []]
    with pytest.raises(ZeroDivisionError):
        va.halda_solve_variants([devs], [(m, "8bit")], k_candidates=[0, 2])
    with pytest.raises(ValueError, match="at most 65535"):
        va.check_variants([(m, "8bit")] * 65536)


def test_variant_major_offsets_against_a_restatement(llama_online_model):
    nv, nf, nd, nk = 5, 3, 10, 9
    o = va.variant_offsets(nv, nf, nd, nk)
    for v in range(nv):
        # the slices of a [n_var, ...] C array: where NumPy puts row v of each output
        for f, shape in (("best_k", (nv, nf)), ("obj_value", (nv, nf)), ("w", (nv, nd)), ("n", (nv, nd)),
                         ("obj_by_k", (nv, nf, nk)), ("status", (nv, nf, nk)), ("x_off", (nv, nf, nk))):
            a = np.arange(int(np.prod(shape))).reshape(shape)
            assert int(o[f][v]) == int(a[v].ravel()[0]), (f, v)
    # the compact layout: the table's own, once per variant, each variant's rows behind the previous one's
    table = fleet_table([synth_devices(2, 0), synth_devices(3, 0), synth_devices(64, 0)], llama_online_model)
    ks = [1, 2, 4, 5, 8, 10, 16, 20, 40]
    xsel = open_x_offsets(table, llama_online_model, ks)
    N = np.repeat(7 * table.sizes() + 1, len(ks))
    ext = int(np.max(xsel + N))
    assert (xsel < 0).any() and (xsel >= 0).any()
    got = va.variant_x_offsets(xsel, ext, 4).reshape(4, -1)
    taken = np.zeros(4 * ext, bool)
    for v in range(4):
        for i, a in enumerate(xsel.tolist()):
            want = -1 if a < 0 else v * ext + a
            assert got[v, i] == want
            if a >= 0:
                assert not taken[want:want + N[i]].any()  # no two instances overlap
                taken[want:want + N[i]] = True
    assert taken.all()  # and nothing is left unused: the variants' rows lie back to back
    assert va.variant_x_offsets(xsel, ext, 1).tolist() == xsel.tolist()


def test_per_variant_constants_equal_those_of_a_table_packed_for_the_variant(llama_online_model):
    m = llama_online_model
    fleets = [synth_devices(M, s) for M, s in ((2, 0), (4, 1), (16, 2), (64, 0))]
    variants = va.model_grid(m, ("4bit", "fp16"), [512, 1 << 20])
    variants += [(m.model_copy(update=u), "8bit") for u in (
        {"b_in": m.b_in * 3}, {"b_out": m.b_out * 5}, {"V": m.V * 2}, {"b_layer": m.b_layer * 2},
        {"f_out": dict(m.f_out, b_1=m.f_out["b_1"] * 7)}, {"f_q": dict(m.f_q, b_1=m.f_q["b_1"] * 3)})]
    table = fleet_table(fleets, variants[0][0])
    got = va.variant_constants(table, variants)
    kappas = set()
    for (mv, _), cs in zip(variants, got):
        own = fleet_table(fleets, mv)
        for f in ("dev_off", "os_class", "flags", "scpu_b1", "sgpu_b1", "T_cpu", "s_disk", "d_avail_ram", "swap"):
            assert np.array_equal(getattr(own, f), getattr(table, f)), f  # the table does not depend on the variant
        want = fleet_constants(own, mv)
        for a, b in zip(cs, want):
            assert a.tobytes() == b.tobytes()
        kappas.add(cs[2].tobytes())
    assert len(kappas) >= 5  # b_in, b_out, V and f_out["b_1"] each move kappa: the constants are per variant


def test_model_structs_are_the_variants_own(llama_online_model):
    from distilp_amd.solver.fleets import HaldaModelC, model_struct
    from distilp_amd.solver.lower import kv_bits_to_factor

    variants = va.model_grid(llama_online_model, ("4bit", "8bit", "fp16"), [512, 65536])
    arr = va.model_structs(variants)
    assert len(arr) == 6 and ctypes.sizeof(arr) == 6 * ctypes.sizeof(HaldaModelC)
    for v, (m, kv) in enumerate(variants):
        s = model_struct(m, kv_bits_to_factor(kv))
        assert bytes(arr[v]) == bytes(s)
    assert len({arr[v].b_prime for v in range(6)}) >= 4  # kv_bits and n_kv reach b_prime


def test_cli_flags_parse():
    from distilp_amd.cli.solver import _parser

    p = _parser()
    a = p.parse_args(["--profile", "hermes_70b"])
    assert a.kv_sweep is None and a.n_kv_sweep is None
    a = p.parse_args(["--profile", "hermes_70b", "--kv-sweep", "4bit", "8bit", "fp16"])
    assert a.kv_sweep == ["4bit", "8bit", "fp16"] and a.n_kv_sweep is None
    a = p.parse_args(["--profile", "hermes_70b", "--n-kv-sweep", "512", "65536", "--quiet"])
    assert a.n_kv_sweep == [512, 65536] and a.kv_sweep is None and a.quiet
    a = p.parse_args(["--profile", "x", "--kv-sweep", "fp16", "--n-kv-sweep", "1"])
    assert (a.kv_sweep, a.n_kv_sweep) == (["fp16"], [1])
    import contextlib
    import io

    for bad in (["--kv-sweep", "3bit"], ["--n-kv-sweep", "many"], ["--kv-sweep"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            p.parse_args(["--profile", "x"] + bad)


def test_variants_kernels_keep_their_siblings_budgets(tmp_path):
    """halda_sweep_variants_kernel: no scratch at four waves per SIMD, like halda_sweep_kernel; the table form
    takes no more registers or scratch than halda_sweep_tables_kernel, whose body it runs."""
    lh.load_library()
    res = kernel_resources(tmp_path)
    r = res["halda_sweep_variants_kernel"]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["vgpr_count"] <= 128, r
    t, b = res["halda_sweep_tables_variants_kernel"], res["halda_sweep_tables_kernel"]
    assert t["vgpr_spill_count"] == 0 and t["vgpr_count"] <= b["vgpr_count"], (t, b)
    assert t["private_segment_fixed_size"] <= b["private_segment_fixed_size"], (t, b)


# ---------------------------------------------------------------- the reference's recorded grid
GOLDEN_FOLDERS = ("llama_3_70b/online", "hermes_70b")


def golden_cases(folder):
    g = load_json("variants.json")
    return g, g["folders"][folder]


@pytest.mark.parametrize("folder", GOLDEN_FOLDERS)
def test_golden_grid_is_not_vacuous(folder):
    g, cases = golden_cases(folder)
    assert g["kv_bits"] == ["4bit", "8bit", "fp16"] and len(g["n_kv"]) == 4
    assert [(c["n_kv"], c["kv_bits"]) for c in cases] == [(n, kv) for n in g["n_kv"] for kv in g["kv_bits"]]
    assert all(c["error"] is None and c["result"] is not None for c in cases)
    plans = {(c["result"]["k"], tuple(c["result"]["w"])) for c in cases}
    assert len(plans) >= 2, plans  # the model variant changes the plan: the grid tests something


def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


@pytest.mark.parametrize("solver", ["exact", "highs"])
@pytest.mark.parametrize("folder", GOLDEN_FOLDERS)
def test_oracle_reproduces_the_recorded_grid(folder, solver):
    """oracle/milp_oracle.py on every (n_kv, kv_bits) of the golden: the same status per k, and the
    reference's result -- (k, w, n, sets) identical, obj_value within 1e-9 relative. A losing k's recorded
    objective is held to the 1e-6 of HiGHS's primal feasibility tolerance instead: the reference's HiGHS may
    leave a slack fractional there (n_kv = 2^20, 8bit, k = 8 of llama_3_70b/online: 1e-6 below the exact
    optimum), which the exact solver does not."""
    g, cases = golden_cases(folder)
    devs, model = fixture_fleet(folder)
    for c in cases:
        m = model.model_copy(update={"n_kv": c["n_kv"]})
        best, per_k = mo.halda_solve_oracle(devs, m, mip_gap=g["mip_gap"], kv_bits=c["kv_bits"], solver=solver)
        ref_k = {r["k"]: r for r in c["per_k"]}
        assert sorted(ref_k) == [r["k"] for r in per_k]
        for r in per_k:
            ref = ref_k[r["k"]]
            assert r["success"] == ref["success"], (c["n_kv"], c["kv_bits"], r["k"])
            if r["success"]:
                assert abs(r["obj_value"] - ref["obj_value"]) <= 1.5e-6 * max(1.0, abs(ref["obj_value"])), (
                    c["n_kv"], c["kv_bits"], r["k"])
        ref = c["result"]
        assert (best["k"], best["w"], best["n"], best["sets"]) == (ref["k"], ref["w"], ref["n"], ref["sets"]), c
        assert close(best["obj_value"], ref["obj_value"])
