"""The oracle side of the tied-fleet suite (tests/tied_cases.py), on the CPU: the conditions the GPU tests of
tests/test_gpu_tied.py rely on hold on the committed case list by the exact oracle alone -- every instance feasible,
nearly all of them non-unique, the pinned re-pricing sound on the oracle's own optima -- and evaluate_plan_np's
bottleneck rule on identical devices."""

import pytest

from . import tied_cases as tc


@pytest.fixture(scope="module")
def inst():
    return tc.instances()


def test_the_kinds_widen_tied_fleets():
    """tied_dicts at M = 16 is what tied_fleets always built (tests/golden/ties.json was made from it), and the
    widened kinds hold the copies they promise."""
    from distilp_amd.synth import synth_fleet

    from .ties import tied_dicts, tied_fleets

    got = tied_fleets(3)
    for s in range(3):
        src = synth_fleet(21000 + s, 16)
        want = [[src[s % 2]] * 16, [src[1]] * 8 + [src[2 + s % 14]] * 8, src[:8] + src[:8]]
        for (kind, devs), dicts in zip(got[3 * s:3 * s + 3], want):
            assert [d.model_dump() for d in devs] == [type(devs[0]).model_validate(q).model_dump() for q in dicts], kind
    for M in (16, 33, 64, 70):
        src = list(range(max(M, 16)))
        h = -(-M // 2)
        assert tied_dicts("copies", src, 1, M) == [1] * M
        assert tied_dicts("two", src, 3, M) == [1] * h + [5] * (M - h)
        assert tied_dicts("half", src, 0, M) == (src[:h] + src[:h])[:M] and len(tied_dicts("half", src, 0, M)) == M


def test_every_instance_is_feasible_and_prices_at_its_optimum(inst):
    assert len(inst) == 18 + 36 + 48 + 6 + 12
    for case, k in inst:
        st, x, b1, _ = tc.exact(case, k)
        assert st == 0, (case, k, st)
        w, n = tc.plan_of(case, k)
        got = tc.pinned_price(case, k, w, n)
        assert got is not None and tc.close(got, tc.objective(case, k)), (case, k, got, tc.objective(case, k))
        tc.check_plan(case, k, w, n, tc.objective(case, k), "oracle")


def test_pinned_price_rejects_and_ranks():
    """A plan outside the bounds or over a device's memory prices None; a feasible non-optimal plan prices above
    the optimum (check_plan would fail on it)."""
    case, k = tc.cases("T16p", kinds=("copies",), scales=(tc.S64,))[0], 1
    w, n = tc.plan_of(case, k)
    assert tc.pinned_price(case, k, [0] + w[1:], n) is None
    assert tc.pinned_price(case, k, w, [v + 1 for v in w]) is None
    worse = [w[0] + 20, w[1] - 20 + sum(w[2:]) - (len(w) - 2)] + [1] * (len(w) - 2)
    assert sum(worse) == sum(w)
    got = tc.pinned_price(case, k, worse, [0] * len(w))
    assert got is None or got > tc.objective(case, k) * (1 + 1e-6)
    with pytest.raises(AssertionError):
        tc.check_plan(case, k, worse, [0] * len(w), tc.objective(case, k))


def test_the_list_is_tied_and_pressured(inst):
    """The shares that make the list worth running: at least 80 % of the instances non-unique by the 1e-7 margin,
    at least half of the scaled ones on a slack, at least 5 with a partial offload; the best-k comparison skipped
    for at most 10 % of the fleets of any class."""
    non_unique = sum(not tc.unique(c, k) for c, k in inst)
    scaled = [(c, k) for c, k in inst if c[2] != 1]
    slack = sum(tc.traits(c, k)[0] for c, k in scaled)
    partial = sum(tc.traits(c, k)[1] for c, k in inst)
    print(f"{len(inst)} instances: {non_unique} non-unique, {slack} of {len(scaled)} scaled on a slack, "
          f"{partial} with a partial offload")
    assert non_unique >= 0.8 * len(inst), (non_unique, len(inst))
    assert slack >= 0.5 * len(scaled), (slack, len(scaled))
    assert partial >= 5, partial
    for cls in tc.CLASSES:
        cs = tc.cases(cls)
        skipped = sum(not tc.best_k_decided(c) for c in cs)
        print(f"{cls}: best k undecided for {skipped} of {len(cs)} fleets")
        assert skipped <= 0.1 * len(cs), (cls, skipped, len(cs))


def test_the_rolled_placement_is_within_reach():
    """At least one case of every class reaches the free optimum from the rolled w0 within 4 loaded layers (the P of
    the frontier tests) and not with none, and so does one of every (class, k) those tests run; w0 is a plan of the
    same total."""
    for cls in tc.CLASSES:
        ps = {(c, k): tc.p_star(c, k) for c, k in tc.instances(tc.cases(cls))}
        for (c, k), p in ps.items():
            assert sum(tc.rolled_w0(c, k)) == tc.L_of(c) // k and min(tc.rolled_w0(c, k)) >= 1
        print(f"{cls}: p* {sorted(ps.values())}")
        assert min(ps.values()) <= 4, (cls, ps)
        assert any(1 <= p <= 4 for p in ps.values()), (cls, ps)
    for cls, k in tc.FRONTIER_RUNS:
        assert any(1 <= tc.p_star(c, k) <= 4 for c in tc.cases(cls)), (cls, k)


def test_evaluate_plan_np_on_the_optima(inst):
    """evaluate_plan_np prices each oracle optimum feasible at the oracle's objective; on `copies` fleets, where H_i
    depends on (w_i, n_i) only, its bottleneck is the lowest index holding the bottleneck's (w, n) pair."""
    from distilp_amd.solver import plans as pl
    from distilp_amd.solver.fleets import fleet_table

    tabs = {}
    for case, k in inst:
        if case not in tabs:
            tabs[case] = fleet_table([tc.devices(case)], tc.model_of(case))
        w, n = tc.plan_of(case, k)
        e = pl.evaluate_plan_np(tabs[case], tc.model_of(case), 0, k, w, n, tc.KV)
        assert e.feasible and e.reason == 0, (case, k, e)
        assert tc.close(e.obj_value, tc.objective(case, k)), (case, k, e.obj_value, tc.objective(case, k))
        if case[1] == "copies":
            b = int(e.bottleneck)
            assert b == min(i for i in range(len(w)) if (w[i], n[i]) == (w[b], n[b])), (case, k, b, w, n)
