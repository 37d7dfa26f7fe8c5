"""The mutation catalogue (tests/csr_mutation_cases.py) on the CPU: one `apply` gives the same mutated MILP in
both forms, and the exact oracle answers every case as include/halda.h promises of the GPU path -- a K case
(structure kept) is solved to HiGHS's verdict and optimum, an R case (structure broken) is rejected, an E case
(a valid MILP the decoder may decline) is rejected or right -- without crashing on any of them. HiGHS's answers
are tests/golden/csr_mutations.json (scipy.optimize.milp at mip_gap = 0, tests/golden/gen_csr_mutations.py);
one test re-solves a sample with the installed scipy. No GPU."""

import numpy as np
import pytest

from oracle import milp_oracle as mo

from . import csr_mutation_cases as mc

OBJ_REL = 1e-9


def _close(a, b):
    return abs(a - b) <= OBJ_REL * max(1.0, abs(b))


@pytest.fixture(scope="module")
def gold():
    return mc.golden()


def test_catalogue_is_complete_and_not_vacuous(gold):
    """Every base holds every kind that applies to it, and at least half of the K cases move the optimum."""
    ks = [rec for b in mc.BASES for rec in gold["bases"][b[0]]["cases"] if rec["cls"] == "K"]
    changed = sum(rec["changed"] for rec in ks)
    print(f"K cases: {len(ks)}, changed: {changed}")
    assert 2 * changed >= len(ks)
    for b in mc.BASES:
        kinds = [rec["kind"] for rec in gold["bases"][b[0]]["cases"]]
        assert len(kinds) == len(set(kinds)) and set(kinds) <= set(mc.kinds_of(b[3])), b
        assert all(mc.KINDS[rec["kind"]] == rec["cls"] for rec in gold["bases"][b[0]]["cases"])
    seen = {rec["kind"] for b in mc.BASES for rec in gold["bases"][b[0]]["cases"]}
    assert seen == set(mc.KINDS), set(mc.KINDS) - seen


@pytest.mark.parametrize("base", mc.BASES, ids=[b[0] for b in mc.BASES])
def test_mutated_csr_equals_mutated_dense_and_oracle_verdicts(llama_online_model, gold, base):
    Pd, Ps = mc.base_dense(llama_online_model, base), mc.base_sparse(llama_online_model, base)
    assert np.array_equal(mc.to_dense(Ps), Pd["A"])
    rows0 = [(c.copy(), v.copy()) for c, v in Ps["rows"]]
    S = mc.Shape(Pd)  # no kind that applies to a device of this base is missing from the golden
    assert [rec["kind"] for rec in gold["bases"][base[0]]["cases"]] == \
        [kind for kind in mc.kinds_of(base[3]) if mc.first_device(kind, S) is not None]
    for rec, ops in mc.cases(llama_online_model, base, gold):
        tag = (base[0], rec["kind"], rec["dev"])
        Qd, Qs = mc.apply(Pd, ops), mc.apply(Ps, ops)
        # the same MILP in both forms, bit for bit
        assert np.array_equal(mc.to_dense(Qs), Qd["A"]), tag
        for f in ("c", "lb", "ub", "integ", "row_lb", "row_ub"):
            assert np.array_equal(Qs[f], Qd[f]), (tag, f)
        # through a batch and back: the mutated instance owns its segment, its clean twin is untouched
        back = mc.split(mc.join([Ps, Qs]))
        assert np.array_equal(mc.to_dense(back[1]), Qd["A"]) and np.array_equal(mc.to_dense(back[0]), Pd["A"]), tag
        st, x, b1, _, _ = mo.exact_solve(mc.to_prob(Qd))
        if rec["cls"] == "R":
            assert st < 0, (tag, st)
            continue
        if rec["cls"] == "E" and st < 0:
            continue
        assert st == (0 if rec["success"] else 2), (tag, st, rec)
        if st == 0:
            assert _close(b1, rec["fun"]), (tag, b1, rec["fun"])
            assert _close(float(np.dot(Qd["c"], x)), rec["fun"]), tag
    # no mutation wrote into the base's shared rows
    assert all(np.array_equal(c, c0) and np.array_equal(v, v0) for (c, v), (c0, v0) in zip(Ps["rows"], rows0))


def test_golden_is_what_highs_answers(llama_online_model, gold):
    """The M = 3 bases again with the installed scipy (HiGHS at mip_gap = 0): the recorded verdicts and optima."""
    pytest.importorskip("scipy")
    for base in [b for b in mc.BASES if b[2] == 3 and not b[4]]:
        Pd = mc.base_dense(llama_online_model, base)
        assert _close(float(mo.highs_solve(mc.to_prob(Pd), mip_gap=0.0).fun), gold["bases"][base[0]]["fun"])
        for rec, ops in mc.cases(llama_online_model, base, gold):
            Q = mc.to_prob(mc.apply(Pd, ops))
            if rec.get("highs") == "error":
                with pytest.raises(ValueError):
                    mo.highs_solve(Q, mip_gap=0.0)
                continue
            res = mo.highs_solve(Q, mip_gap=0.0)
            assert bool(res.success) == rec["success"], (base[0], rec)
            if res.success:
                assert abs(float(res.fun) - rec["fun"]) <= 1e-6 * max(1.0, abs(rec["fun"])), (base[0], rec)


def test_negative_w_lower_bound_does_not_corrupt_the_heap(llama_online_model):
    """lb(w_0) = -1 used to index the oracle's pair table at w = -1 (free(): invalid pointer). It is rejected
    now, as is a negative n bound; bounds of +inf and beyond the int range are clamped, not cast."""
    p = mo.lower_dense(mc.devices(0, 4), llama_online_model, 1, mc.KV)
    st0, _, b0, _, _ = mo.exact_solve(p)
    assert st0 == 0
    for j, v in ((0, -1.0), (4, -1.0), (0, -1e300)):
        q = dict(p, lb=p["lb"].copy())
        q["lb"][j] = v
        assert mo.exact_solve(q)[0] < 0
    q = dict(p, ub=p["ub"].copy(), lb=p["lb"].copy())
    q["ub"][0], q["ub"][4 + 1], q["ub"][2 * 4] = np.inf, 1e300, 1e300  # w_0, n_1, s1_0
    st, _, b1, _, _ = mo.exact_solve(q)
    assert st == 0 and b1 <= b0 + 1e-12
    q["lb"][1] = 1e300
    assert mo.exact_solve(q)[0] == 2
