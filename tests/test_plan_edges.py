"""The plan-edge shape list itself (tests/plan_edge_cases.py), on the CPU: every shape is there once on each
side of its threshold, the threshold stated as plain arithmetic on (sizes, L, ks, nf); every instance with room is
feasible for the exact oracle and at least 80 % of them have a unique optimum; HiGHS and the NumPy plan
evaluation agree with the oracle on them. No GPU (halda_lds_bytes, which sizes the two LDS-budget shapes, is
host arithmetic of libhalda)."""

from fractions import Fraction

import numpy as np

from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table
from oracle import milp_oracle as mo

from . import plan_edge_cases as pe


def test_every_shape_sits_once_on_each_side_of_its_threshold():
    shapes = pe.shapes()
    names = [s.name for s in shapes]
    assert len(set(names)) == len(names)
    keys = [(s.part, s.sizes, s.L, s.ks, tuple(sorted(s.launch))) for s in shapes]
    assert len(set(keys)) == len(keys), "a shape is listed twice"
    # the shapes come in pairs: one threshold, the same sizes, "at" then "past"
    assert len(shapes) % 2 == 0
    for at, past in zip(shapes[0::2], shapes[1::2]):
        assert (at.side, past.side) == ("at", "past") and at.threshold == past.threshold, (at.name, past.name)
        assert at.part == past.part and at.sizes == past.sizes, (at.name, past.name)
        for sh in (at, past):
            for nf in (sh.launch or {0: ()}):
                assert pe.predicate(sh, nf) == (sh.side == "at"), (sh.name, nf)
            assert 1 <= len(sh.fleets) <= 4 or sh.name.startswith("loo_"), sh.name
            assert {f[0] for f in sh.fleets} == set(sh.sizes), sh.name
            scales = {f[1] for f in sh.fleets}
            assert Fraction(1) in scales and scales & {pe.S16, pe.S32}, sh.name
    assert {s.part for s in shapes} == set("ABCDE")
    # the thresholds' two sides are adjacent integers
    by = {s.name: s for s in shapes}
    for a, b in (("m64_r64", "m64_r65"), ("mix_r64", "mix_r65"), ("m1_r64", "m1_r65"), ("m2_r64", "m2_r65"),
                 ("lds_fits", "lds_over"), ("alone_r64", "alone_r65"), ("loo_r64", "loo_r65")):
        assert by[b].L == by[a].L + 1, (a, b)
    assert [by[n].L - min(by[n].sizes) + 1 for n in ("m64_r64", "mix_r64", "m1_r64", "m2_r64", "loo_r64")] == [64] * 5
    assert (max(by["nf64"].launch), min(by["nf65"].launch)) == (64, 65) and set(by["nf65"].launch) == {65, 66, 67}
    assert (len(by["k64"].ks), len(by["k65"].ks)) == (64, 65)
    open_k = lambda s: pe.open_k(s.sizes, s.L, s.ks)  # noqa: E731
    assert [open_k(by[n]) for n in ("slots16", "slots17", "one_slot", "two_slots")] == [16, 17, 1, 2]
    assert open_k(by["no_room"]) == 1 and by["no_room"].ks[0] == 1 and open_k(by["closed_k"]) == 1
    assert by["no_room"].L - 16 + 1 == 64  # no table launch behind its register launch
    # the k-slot launch's tables: 24 KiB under the budget with k = 2, 3 and 11 KiB over it with k = 4 added
    assert pe.kslot_table_bytes(*by["kslot_fits"][2:5]) == 139264 and pe.kslot_table_bytes(*by["kslot_over"][2:5]) == 175104
    # every launch kind is expected somewhere, the register launch with a table launch behind it at nf > 64
    kinds = {(nf > 64, launch) for s in shapes for nf, launch in s.launch.items()}
    assert {(False, pe.REG), (True, pe.REG), (False, pe.TABLES), (True, pe.TABLES), (True, pe.REG_GATED),
            (False, pe.REG_GATED), (True, pe.KSLOT), (True, pe.SEG), (False, pe.CSR)} <= kinds
    # part B also runs with the k-slot kernel off: the segment kernel on one side of the batch-size and
    # k-count thresholds, the table kernel on the other
    assert [by[n].seg[nf] for n, nf in (("nf64", 64), ("nf65", 65), ("nf65", 67), ("slots16", 66), ("slots17", 66))
            ] == [pe.TABLES, pe.SEG, pe.SEG, pe.SEG, pe.TABLES]
    assert all(set(s.seg) == set(s.dp) == set(s.launch) for s in shapes if s.part == "B")
    # a batch repeats the distinct fleets, every second copy reversed
    b = pe.batch(by["nf65"], 67)
    d = pe.cases_of(by["nf65"])
    assert b[:4] == d and b[4:8] == d[::-1] and b[8:12] == d and len(b) == 67 and set(b) == set(d)


def test_instances_are_feasible_and_mostly_unique():
    """Conditions on the list, not measurements: every instance with room feasible, at least 80 % unique.
    Measured: 432 instances, 432 feasible, 432 unique (100 %), 196 with a slack or t column in use."""
    inst = pe.instances()
    sh = pe.shares(inst)
    print("plan edges:", sh)
    assert sh["instances"] >= 400 and sh["feasible"] == sh["instances"], sh
    assert sh["unique"] >= 0.8 * sh["feasible"], sh
    for s in pe.shapes():  # every shape has pressured optima: a slack or a t column in use
        one = pe.shares(pe.instances([s]))
        assert one["slack_or_t"] >= 1 and one["feasible"] == one["instances"], (s.name, one)


def _highs_agrees(case, k, res):
    st, xo, b1, _ = pe.exact(case, k)
    if res.success != (st == 0):
        return False
    if st != 0:
        return True
    M, p = case[0], pe.problem(case, k)
    if not pe.close(float(np.dot(p["c"], res.x)), b1):
        return False
    return not pe.unique(case, k) or np.array_equal(np.rint(res.x[:2 * M]), xo[:2 * M])


def test_exact_oracle_matches_highs_on_the_small_shapes():
    """HiGHS (mip_gap None) against the exact oracle on at most 60 instances of at most 16 devices: status, c.x
    within 1e-9 relative, where unique (w, n). An instance where HiGHS with presolve departs is compared with the
    presolve-off answer; every exception class is counted and capped at 5 % (tests/test_pressure.py)."""
    from scipy.optimize import Bounds, LinearConstraint, milp

    small = [(c, k) for c, k in pe.instances() if c[0] <= 16]
    sub = small[::-(-len(small) // 60)]
    assert 40 <= len(sub) <= 60 and {c[0] for c, _ in sub} == {1, 2, 4, 16}, len(sub)
    assert {c[3] for c, _ in sub} >= {64, 80, 130, 200}
    nopre = []
    for case, k in sub:
        p = pe.problem(case, k)
        if _highs_agrees(case, k, mo.highs_solve(p, mip_gap=None)):
            continue
        nopre.append((case, k))
        cons = [LinearConstraint(p["A_ub"], -np.inf, p["b_ub"]), LinearConstraint(p["A_eq"], p["b_eq"], p["b_eq"])]
        res = milp(c=p["c"], integrality=p["integrality"], bounds=Bounds(p["lb"], p["ub"]), constraints=cons,
                   options={"time_limit": 3600.0, "presolve": False})
        assert _highs_agrees(case, k, res), (case, k)
    print(f"HiGHS = exact oracle on {len(sub) - len(nopre)} of {len(sub)}; presolve-off class: {nopre}")
    assert len(nopre) <= 0.05 * len(sub), nopre


def test_numpy_plan_evaluation_prices_the_optima_of_part_e():
    """evaluate_plan_np on the oracle's optimum of every instance of part E (the plans and bounds tests start
    from them): feasible, at the oracle's objective within 1e-9, with the oracle's slack and t columns."""
    count = 0
    for sh in pe.shapes():
        if sh.part != "E":
            continue
        model = pe.model_of(sh.L)
        for case in pe.cases_of(sh):
            st, xo, _, _ = pe.exact(case, 1)
            assert st == 0
            M = case[0]
            t = fleet_table([pe.devices(case)], model)
            e = pl.evaluate_plan_np(t, model, 0, 1, np.rint(xo[:M]), np.rint(xo[M:2 * M]), pe.kv_factor(case[4]))
            assert e.feasible and e.reason == 0, (case, e.reason)
            assert pe.close(e.obj_value, pe.objective(case, 1)), (case, e.obj_value, pe.objective(case, 1))
            pe.check_x(e.x, case, 1, "evaluate_plan_np")
            count += 1
    assert count == 2 * 2 + 2 * 2 * len(pe.LOO_DROPS)
