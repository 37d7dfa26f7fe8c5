"""The milp() replacement on mutated CSRs (tests/csr_mutation_cases.py): include/halda.h promises that a matrix
without the HALDA structure is rejected with HALDA_STATUS_UNSUPPORTED, never approximated. Every base's cases
run as the instances of ONE batch through halda_solve_batch, halda_solve_batch_device and
halda_solve_batch_device_settled (all-zero flags: the settled k = 1 kernel's own screen):

  K (structure kept)     the status is HiGHS's verdict; when optimal, obj_lin and the host-side c.x are within
                         1e-9 relative of HiGHS's optimum and x is integral where flagged, inside the mutated
                         bounds and satisfies every mutated row within 1e-6 layers (README's boundary rule);
  R (structure broken)   exactly HALDA_STATUS_UNSUPPORTED;
  E (may be declined)    UNSUPPORTED, or the K rule. Never a third answer.

The k = 1 fast decode (decode_k1) has its own copy of the cycle-row checks. Its test for w entered twice is
reached by cyc_dup_w alone, an E kind on k = 1 bases where the cycle rows do not move the objective: were that
line gone, the case would be caught by the row check on the returned z and C (the row would be decoded with half
its w coefficient), not by obj_lin.

Reads only tests/golden/csr_mutations.json (HiGHS at mip_gap = 0, recorded on the CPU)."""

import numpy as np
import pytest

from distilp_amd.solver._libhalda import (STATUS_INFEASIBLE, STATUS_OPTIMAL, STATUS_TOO_LARGE, STATUS_UNSUPPORTED,
                                          get_context)

from . import csr_mutation_cases as mc

pytestmark = pytest.mark.gpu

OBJ_REL = 1e-9
ROW_TOL = 1e-6  # layers
FIELDS = ("n_cols", "n_rows", "csr_off", "col_off", "row_off", "row_ptr", "col_idx", "val", "c", "col_lb", "col_ub",
          "row_lb", "row_ub", "integrality")
_cache = {}


def _close(a, b):
    return abs(a - b) <= OBJ_REL * max(1.0, abs(b))


def _base(model, base):
    """(records, dense forms, batch, host result) of a base: instance 0 clean, then one instance per case."""
    if base[0] not in _cache:
        Pd, Ps = mc.base_dense(model, base), mc.base_sparse(model, base)
        cs = mc.cases(model, base)
        dense = [Pd] + [mc.apply(Pd, ops) for _, ops in cs]
        batch = mc.join([Ps] + [mc.apply(Ps, ops) for _, ops in cs])
        _cache[base[0]] = ([None] + [rec for rec, _ in cs], dense, batch, get_context(0).solve(batch))
    return _cache[base[0]]


def _x_of(batch, x, j):
    return x[int(batch.col_off[j]):int(batch.col_off[j]) + int(batch.n_cols[j])]


def _assert_solves(tag, Q, x, obj_lin, fun):
    """The K rule for an instance the GPU called optimal."""
    N = len(Q["c"])
    M = (N - 1) // 7
    assert _close(obj_lin, fun), (tag, obj_lin, fun)
    assert _close(float(np.dot(Q["c"], x)), fun), (tag, float(np.dot(Q["c"], x)), fun)
    flagged = Q["integ"].astype(bool)
    assert np.array_equal(x[flagged], np.round(x[flagged])), tag
    assert np.all(x >= Q["lb"]) and np.all(x <= Q["ub"]), (tag, np.flatnonzero((x < Q["lb"]) | (x > Q["ub"])))
    A, rub, rlb = Q["A"], Q["row_ub"], Q["row_lb"]
    assert rlb[-1] <= float(A[-1] @ x) <= rub[-1], tag  # sum w = W, in integers
    for r in range(A.shape[0] - 1):
        a = A[r]
        resid = float(a @ x) - rub[r]
        if a[7 * M] != 0.0:  # a cycle row: continuous z and C, no integer column to absorb a shortfall
            assert resid <= 1e-9 * max(1.0, float(np.abs(a * x).sum()), abs(rub[r])), (tag, r, resid)
            continue
        slack = np.abs(a[2 * M:6 * M])
        scale = float(slack.max()) if slack.any() else float(np.abs(a).max())
        assert resid <= ROW_TOL * (scale if scale > 0.0 else 1.0), (tag, r, resid / (scale or 1.0))


def _assert_verdict(tag, rec, Q, status, x, obj_lin):
    if rec["cls"] == "R":
        assert status == STATUS_UNSUPPORTED, (tag, status)
        return
    if rec["cls"] == "E" and status == STATUS_UNSUPPORTED:
        return
    assert status == (STATUS_OPTIMAL if rec["success"] else STATUS_INFEASIBLE), (tag, status, rec)
    if status == STATUS_OPTIMAL:
        _assert_solves(tag, Q, x, obj_lin, rec["fun"])


@pytest.mark.parametrize("base", mc.BASES, ids=[b[0] for b in mc.BASES])
def test_every_case_is_solved_or_rejected(llama_online_model, base):
    recs, dense, batch, res = _base(llama_online_model, base)
    assert res.status[0] == STATUS_OPTIMAL
    _assert_solves((base[0], "clean"), dense[0], _x_of(batch, res.x, 0), float(res.obj_lin[0]),
                   mc.golden()["bases"][base[0]]["fun"])
    verdicts = {}
    for j in range(1, batch.n_inst):
        rec = recs[j]
        verdicts.setdefault(rec["cls"], []).append(int(res.status[j]))
        _assert_verdict((base[0], rec["kind"], rec["dev"]), rec, dense[j], int(res.status[j]), _x_of(batch, res.x, j),
                        float(res.obj_lin[j]))
    print(base[0], {cls: {s: v.count(s) for s in sorted(set(v))} for cls, v in verdicts.items()})
    assert STATUS_UNSUPPORTED not in verdicts["K"]


def _device_solve(batch, settled):
    """halda_solve_batch_device (settled None) or _settled on the batch in HBM: the outputs as NumPy arrays."""
    import torch

    dev = torch.device("cuda", 0)
    keep = {f: torch.from_numpy(np.ascontiguousarray(getattr(batch, f))).to(dev) for f in FIELDS}
    n = batch.n_inst
    out = {"status": torch.full((n,), 7, dtype=torch.int32, device=dev),
           "x": torch.full((batch.total_cols,), -3.0, dtype=torch.float64, device=dev),
           "obj_lin": torch.full((n,), -5.0, dtype=torch.float64, device=dev),
           "dual_bound": torch.full((n,), -5.0, dtype=torch.float64, device=dev),
           "gap": torch.full((n,), -5.0, dtype=torch.float64, device=dev),
           "nodes": torch.full((n,), -9, dtype=torch.int64, device=dev)}
    hint = None if settled is None else torch.from_numpy(settled).to(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    get_context(0).solve_device({f: t.data_ptr() for f, t in keep.items()}, batch,
                                {f: t.data_ptr() for f, t in out.items()}, stream=stream.cuda_stream,
                                settled=None if hint is None else hint.data_ptr())
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same_results(batch, got, want_status, want_x, want_obj, which=None):
    which = range(batch.n_inst) if which is None else which
    for j in which:
        assert got["status"][j] == want_status[j], (j, got["status"][j], want_status[j])
        assert got["obj_lin"][j] == want_obj[j] or (np.isnan(got["obj_lin"][j]) and np.isnan(want_obj[j])), j
        if want_status[j] == STATUS_OPTIMAL:  # x is written for OPTIMAL instances only
            assert np.array_equal(_x_of(batch, got["x"], j), _x_of(batch, want_x, j)), j


@pytest.mark.parametrize("base", mc.BASES, ids=[b[0] for b in mc.BASES])
def test_device_and_settled_entries_give_the_host_entry_bits(llama_online_model, base):
    """The same mutated batch through halda_solve_batch_device and, with an all-zero flag array, through
    halda_solve_batch_device_settled (no screen launch: halda_solve_k1_settled_kernel screens on its way)."""
    _, _, batch, res = _base(llama_online_model, base)
    _assert_same_results(batch, _device_solve(batch, None), res.status, res.x, res.obj_lin)
    _assert_same_results(batch, _device_solve(batch, np.zeros(batch.n_inst, np.uint8)), res.status, res.x, res.obj_lin)


@pytest.mark.parametrize("base", mc.BASES, ids=[b[0] for b in mc.BASES])
def test_a_mutated_fleet_leaves_its_neighbours_alone(llama_online_model, base):
    """Three fleets, each with its instance at the base's k twice (one CSR segment for both, permuted where the
    base is); the middle fleet is the base and its two instances are mutated, one by an R case and one by a K
    case that moves the optimum. The mutated instances read UNSUPPORTED and HiGHS's mutated optimum, and the
    other fleets' status, x and obj_lin are those of the all-clean batch, bit for bit (the screen reuses the
    equality row of the previous open instance; a mutated instance owns its CSR segment)."""
    _, seed, M, k, perm = base
    ctx = get_context(0)
    forms = []
    for s in (seed + 100, seed, seed + 200):
        P = mc.base_sparse(llama_online_model, ("", s, M, k, perm))
        forms += [P, dict(P)]  # two instances on one `rows` list
    clean = mc.join(forms)
    assert clean.csr_off[0] == clean.csr_off[1] != clean.csr_off[2] == clean.csr_off[3]
    cs = mc.cases(llama_online_model, base)
    # a broken equality row on every other base (the field the screen caches), a broken cycle row on the rest
    r_kind = "eq_W_fractional" if mc.BASES.index(base) % 2 else "cyc_z_coef"
    r_ops = next(ops for rec, ops in cs if rec["kind"] == r_kind)
    k_rec, k_ops = next((rec, ops) for rec, ops in cs if rec["cls"] == "K" and rec["changed"] and rec["success"])
    forms[2], forms[3] = mc.apply(forms[2], r_ops), mc.apply(forms[3], k_ops)
    want, got = ctx.solve(clean), ctx.solve(mc.join(forms))
    assert list(want.status) == [STATUS_OPTIMAL] * 6
    assert got.status[2] == STATUS_UNSUPPORTED and got.status[3] == STATUS_OPTIMAL
    assert _close(float(got.obj_lin[3]), k_rec["fun"]) and not _close(float(want.obj_lin[3]), k_rec["fun"])
    _assert_same_results(clean, {"status": got.status, "x": got.x, "obj_lin": got.obj_lin}, want.status, want.x,
                         want.obj_lin, which=(0, 1, 4, 5))


def test_instances_beyond_the_shape_summary_are_too_large(llama_online_model):
    """Device entry, the shape summary sized for the batch's 3-device instances alone: the 16-device fleet's
    instances read HALDA_STATUS_TOO_LARGE, the others are those of a correctly sized call, bit for bit -- by
    the screen launch and by the settled kernel's screen."""
    from distilp_amd.solver.batch import assemble
    from distilp_amd.solver.lower import lower_fleet

    fleets = [mc.devices(0, 3), mc.devices(2, 16), mc.devices(3, 3)]
    full, refs = assemble([lower_fleet(d, llama_online_model, "4bit") for d in fleets], [[1, 2]] * 3)
    forms = mc.split(full)
    small = [j for j, r in enumerate(refs) if r.fleet != 1]
    short = mc.join(forms, summary=mc.shape_summary([forms[j] for j in small]))
    assert short.max_cols == 22 and full.max_cols == 7 * 16 + 1
    for settled in (None, np.zeros(full.n_inst, np.uint8)):
        want, got = _device_solve(full, settled), _device_solve(short, settled)
        assert list(want["status"]) == [STATUS_OPTIMAL] * 6
        assert [int(got["status"][j]) for j in (2, 3)] == [STATUS_TOO_LARGE] * 2
        _assert_same_results(full, got, want["status"], want["x"], want["obj_lin"], which=small)
