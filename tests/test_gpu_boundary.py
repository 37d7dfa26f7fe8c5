"""GPU parity on the boundary goldens (tests/golden/boundary.json, see tests/boundary.py): capacity rows a few
bytes short of a whole number of layers, every row kind, inside and outside the window in which the reference
takes the integer slack as 0. Compared with the goldens only (never with the oracle): status per k, (w, n) per
k, obj_by_k within 1e-9 of the reference's objective at its rounded integer columns, and (k, w, n) of the
sweep; reference_failure cases against the presolve-off record; reference_unstable cases against the HiGHS
answer their `match` names, the tied ones among them by objective."""

import collections

import numpy as np
import pytest

from distilp_amd.solver._libhalda import STATUS_INFEASIBLE, STATUS_OPTIMAL, get_context
from distilp_amd.solver.batch import assemble, settled_instances
from distilp_amd.solver.fleets import fleet_table, solve_table
from distilp_amd.solver.lower import kv_bits_to_factor, lower_fleet

from . import boundary as bd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches():
    """Cases grouped into batches of one model, kv and fleet size: [(model, kv_bits, ks, [(g, c, devs)])]."""
    by = collections.OrderedDict()
    for g, c in bd.all_cases():
        by.setdefault((g["fleet"] if "synth" not in g["fleet"] else "synth", g["kv_bits"], len(g["sets"]["M1"])
                       + len(g["sets"]["M2"]) + len(g["sets"]["M3"]), tuple(g["ks"])), []).append((g, c, bd.devices(g, c)))
    return [(bd.base_fleet(items[0][0]["fleet"])[1], key[1], list(key[3]), items) for key, items in by.items()]


def _n_window():
    """In-window cases of the file that have an answer to reproduce."""
    return sum(bd.in_window(g, c) for g, c in bd.all_cases() if bd.expected(g, c) is not None)


def _per_k_of_table(res, f, M, ks):
    out = []
    for j, k in enumerate(ks):
        ok = int(res.status[f, j]) == STATUS_OPTIMAL
        assert ok or int(res.status[f, j]) == STATUS_INFEASIBLE, (f, k, int(res.status[f, j]))
        r = {"k": k, "success": ok}
        if ok:
            x = res.x[f, j]
            r.update(w=[int(round(v)) for v in x[:M]], n=[int(round(v)) for v in x[M:2 * M]],
                     obj_value=float(res.obj_by_k[f, j]))
        out.append(r)
    return out


def _check(items, per_k_of, best_of=None):
    n_win = n_inf = 0
    for f, (g, c, devs) in enumerate(items):
        tag = (g["fleet"], g["kv_bits"], g["device"], g["row"], g["j"], c["delta"])
        got = per_k_of(f)
        want = bd.expected(g, c)
        if want is None:
            bd.check_tied(got, g, c, tag)
            continue
        res, want_k = want
        bd.check_per_k(got, want_k, tag)
        n_inf += sum(not r["success"] for r in want_k)
        n_win += bd.in_window(g, c)
        if best_of is not None:
            assert best_of(f) == (res["k"], res["w"], res["n"]), tag
    return n_win, n_inf


@pytest.mark.parametrize("path", ["fused", "csr", "wave", "seg"])
def test_solve_table_matches_the_boundary_goldens(batches, path):
    """Every case as one batch per (model, kv, fleet size) through halda_solve_fleets: the default fused sweep
    (the k-slot kernel for the batches of more than 64 small fleets), the CSR pipeline (decode_cap_row), one
    fleet per wave, and the segment kernel (field_rec). Bound-infeasible k stay infeasible."""
    ctx = get_context(0)
    ctx.set_fleets_path(path)
    n_win = n_inf = 0
    try:
        for model, kv, ks, items in batches:
            fleets = [devs for _, _, devs in items]
            M = len(fleets[0])
            table = fleet_table(fleets, model)
            res = solve_table(table, model, ks, kv_bits_to_factor(kv), want_x=True)

            def best_of(f):
                a, b = int(table.dev_off[f]), int(table.dev_off[f + 1])
                return int(res.best_k[f]), [int(v) for v in res.w[a:b]], [int(v) for v in res.n[a:b]]

            a, b = _check(items, lambda f: _per_k_of_table(res, f, M, ks), best_of)
            n_win, n_inf = n_win + a, n_inf + b
    finally:
        ctx.set_fleets_path(True)
    assert n_win == _n_window() and n_inf > 0, (n_win, n_inf)


def test_path_b_csr_matches_the_boundary_goldens(batches):
    """The lowered CSR of every case through halda_solve_batch (the milp() replacement): status, w and n per k
    equal the golden's, c.x + constants within 1e-9 of the reference's objective; and through
    halda_solve_batch_device_settled with the lowering's own flags, whose results equal those bit for bit."""
    import torch

    ctx = get_context(0)
    dev = torch.device("cuda", 0)
    n_win = 0
    for model, kv, ks, items in batches:
        lowered = [lower_fleet(devs, model, kv) for _, _, devs in items]
        batch, refs = assemble(lowered, [ks] * len(lowered))
        res = ctx.solve(batch)
        M = len(items[0][2])
        nk = len(ks)

        def per_k(f):
            out = []
            for j, k in enumerate(ks):
                idx = f * nk + j
                ref = refs[idx]
                assert (ref.fleet, ref.k) == (f, k)
                ok = int(res.status[idx]) == STATUS_OPTIMAL
                assert ok or int(res.status[idx]) == STATUS_INFEASIBLE
                r = {"k": k, "success": ok}
                if ok:
                    x = res.x[ref.col_off:ref.col_off + ref.n_cols]
                    r.update(w=[int(round(v)) for v in x[:M]], n=[int(round(v)) for v in x[M:2 * M]],
                             obj_value=lowered[f].objective_value(ref.c, x))
                out.append(r)
            return out

        n_win += _check(items, per_k)[0]
        # the same batch through halda_solve_batch_device_settled with the lowering's own flags
        got = bd.settled_device_solve(ctx, batch, settled_instances(batch), dev, torch.cuda.Stream(dev))
        assert np.array_equal(got["status"], res.status)
        assert np.array_equal(got["obj_lin"], res.obj_lin)
        for i in np.flatnonzero(res.status == STATUS_OPTIMAL):
            a, b = int(batch.col_off[i]), int(batch.col_off[i] + batch.n_cols[i])
            assert np.array_equal(got["x"][a:b], res.x[a:b])
    assert n_win == _n_window()


def test_single_fleet_halda_solve_matches_the_boundary_goldens(capsys):
    """halda_solve (the resident wave) on a subset: for the first group of every row kind the cases at -10 B,
    0.5 T, 0.9 T, 1.1 T and 10^4 B that have an answer to reproduce, and the first reference_failure cases."""
    from distilp_amd.solver import halda_solve

    picked, seen = [], set()
    for g in bd.golden()["groups"]:
        if g["row"] in seen:
            continue
        seen.add(g["row"])
        T = g["T"]
        targets = [-10.0, round(0.5 * T, 3), round(0.9 * T, 3), round(1.1 * T, 3), 10000.0]
        picked += [(g, c) for c in g["cases"] if c["delta_target"] in targets and bd.expected(g, c) is not None]
    picked += [(g, c) for g, c in bd.all_cases() if bd.klass(c) == "reference_failure"][:3]
    assert seen == set(bd.KINDS) and sum(bd.in_window(g, c) for g, c in picked) >= len(bd.KINDS)
    for g, c in picked:
        tag = (g["fleet"], g["kv_bits"], g["device"], g["row"], g["j"], c["delta"])
        res, per_k = bd.expected(g, c)
        _, model = bd.base_fleet(g["fleet"])
        r = halda_solve(bd.devices(g, c), model, mip_gap=1e-4, plot=False, kv_bits=g["kv_bits"])
        assert (r.k, r.w, r.n, r.sets) == (res["k"], res["w"], res["n"], g["sets"]), tag
        want = next(q for q in per_k if q["k"] == res["k"])["obj_value_rint"]
        assert bd.obj_close(r.obj_value, want), (tag, r.obj_value, want)
    capsys.readouterr()


def test_kslot_kernel_and_group_launch_on_the_16_device_cases(batches):
    """The M = 16 cases repeated past 64 fleets, so that the default path takes the k-slot kernel; then the
    steps / group launch over two resident copies of the same table, whose results equal solve_table's bit
    for bit."""
    import torch

    from distilp_amd.solver.fleets import DeviceFleetTable, PlanGroup

    ctx = get_context(0)
    dev = torch.device("cuda", 0)
    ran = 0
    for model, kv, ks, items in batches:
        if len(items[0][2]) != 16:
            continue
        ran += 1
        reps = -(-65 // len(items)) + 1
        big = items * reps
        assert len(big) > 64
        table = fleet_table([devs for _, _, devs in big], model)
        kvf = kv_bits_to_factor(kv)
        res = solve_table(table, model, ks, kvf, want_x=True)
        assert "halda_sweep_kslot_kernel" in ctx.last_fleet_ms(), ctx.last_fleet_ms()
        _check(big, lambda f: _per_k_of_table(res, f, 16, ks))
        want = solve_table(table, model, ks, kvf)
        tabs = [DeviceFleetTable(table, model, ks, kvf, dev, want_per_k=True) for _ in range(2)]
        group = PlanGroup(tabs, ctx)
        group.launch(0, 2, torch.cuda.Stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        for t in tabs:
            assert np.array_equal(t.out["best_k"].cpu().numpy(), want.best_k)
            assert np.array_equal(t.out["obj_value"].cpu().numpy(), want.obj_value)
            assert np.array_equal(t.out["w"].cpu().numpy(), want.w) and np.array_equal(t.out["n"].cpu().numpy(), want.n)
            assert np.array_equal(t.out["status"].cpu().numpy(), want.status.ravel())
            assert np.array_equal(t.out["obj_by_k"].cpu().numpy(), want.obj_by_k.ravel())
        group.close()
    assert ran == 2  # kv 4bit and fp16
