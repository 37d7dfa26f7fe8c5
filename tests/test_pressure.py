"""Memory-pressured fleets on the CPU (tests/pressure_cases.py): the case list is in the pressured regime and
the unscaled fleets are not; the exact oracle, HiGHS, the NumPy plan evaluation and the host lowering agree on
it; both oracle solvers reproduce the reference's recorded results (tests/golden/pressure.json). No GPU."""

from fractions import Fraction

import numpy as np
import pytest

from distilp_amd.solver import plans as pl
from distilp_amd.solver.fleets import fleet_table
from distilp_amd.solver.lower import lower_fleet
from oracle import milp_oracle as mo

from . import pressure_cases as pc
from .conftest import load_json
from .test_lowering import _check


def test_pressure_cases_are_pressured():
    """The floors are conditions on the case list, not measurements: slack >= 90 %, t >= 25 %, partial offload
    >= 25 %, unique >= 95 % of the feasible instances. Measured: 94.9 %, 31.4 %, 48.3 %, 100 % of 408."""
    inst = pc.instances()
    sh = pc.shares(inst)
    print("pressured:", sh)
    assert sh["instances"] == 408 and sh["feasible"] >= 400, sh
    for key, floor in pc.FLOORS.items():
        assert sh[key] >= floor * sh["feasible"], (key, floor, sh)
    # every (M, scale) class and both kv widths are there
    assert {(c[0], c[1]) for c, _ in inst} == set(pc.CLASSES) and {c[3] for c, _ in inst} == {"4bit", "fp16"}
    # the unscaled fleets of the same seeds: no slack, no t, no partial offload in any optimum
    for M in (16, 64):
        un = pc.shares(pc.instances([(M, Fraction(1), s, "4bit") for s in range(16)]))
        print(f"unscaled M = {M}:", un)
        assert un["feasible"] == un["instances"] == 16 * len(pc.ks_of(M)), un
        assert (un["slack"], un["t"], un["partial"]) == (0, 0, 0), (M, un)


def _highs_agrees(case, k, res):
    """HiGHS's answer `res` on (case, k) against the exact oracle: status, rounded (w, n) where unique, c.x."""
    st, xo, b1, _ = pc.exact(case, k)
    if res.success != (st == 0):
        return False
    if st != 0:
        return True
    M, p = case[0], pc.problem(case, k)
    if not pc.close(float(np.dot(p["c"], res.x)), b1):
        return False
    return not pc.unique(case, k) or np.array_equal(np.rint(res.x[:2 * M]), xo[:2 * M])


def test_exact_oracle_matches_highs_under_pressure():
    """HiGHS (mip_gap None) against the exact oracle on every M = 2, 3, 5 case and seeds 0..3 of M = 16, 33, 64.
    A case where HiGHS with presolve departs (a fractional slack or a presolve flip) is compared
    with the presolve-off answer, counted, and capped at 5 % of the subset."""
    from scipy.optimize import Bounds, LinearConstraint, milp

    sub = pc.instances(pc.cases(Ms=(2, 3, 5)) + pc.cases(Ms=(16, 33, 64), seeds=range(4)))
    assert len(sub) >= 250
    nopre = []
    for case, k in sub:
        p = pc.problem(case, k)
        if _highs_agrees(case, k, mo.highs_solve(p, mip_gap=None)):
            continue
        nopre.append((case, k))
        cons = [LinearConstraint(p["A_ub"], -np.inf, p["b_ub"]), LinearConstraint(p["A_eq"], p["b_eq"], p["b_eq"])]
        res = milp(c=p["c"], integrality=p["integrality"], bounds=Bounds(p["lb"], p["ub"]), constraints=cons,
                   options={"time_limit": 3600.0, "presolve": False})
        assert _highs_agrees(case, k, res), (case, k)
    print(f"HiGHS = exact oracle on {len(sub) - len(nopre)} of {len(sub)}; presolve-off class: {nopre}")
    assert len(nopre) <= 0.05 * len(sub), nopre


@pytest.fixture(scope="module")
def tables():
    """{case: one-fleet FleetTable} of the kv 4bit cases."""
    return {c: fleet_table([pc.devices(c[2], c[0], c[1])], pc.our_model())
            for c in pc.cases(kvs=("4bit",)) + list(pc.NEIGHBOUR_EXTRA)}


def test_numpy_plan_evaluation_of_the_optimum(tables):
    """evaluate_plan_np on the oracle's optimum of every case (both kv widths): feasible, the oracle's
    objective within 1e-9, the oracle's slack and t columns, and the bottleneck = the device attaining max_i H_i
    recomputed here from the dense cycle rows."""
    model = pc.our_model()
    count = 0
    for case, k in pc.instances():
        st, xo, _, _ = pc.exact(case, k)
        if st != 0:
            continue
        M, p = case[0], pc.problem(case, k)
        t = tables[case] if case in tables else fleet_table([pc.devices(case[2], M, case[1])], model)
        e = pl.evaluate_plan_np(t, model, 0, k, np.rint(xo[:M]), np.rint(xo[M:2 * M]), pc.kv_factor(case[3]))
        assert e.feasible and e.reason == 0, (case, k, e.reason)
        assert pc.close(e.obj_value, pc.objective(case, k)), (case, k, e.obj_value, pc.objective(case, k))
        pc.check_x(e.x, case, k, "evaluate_plan_np")
        # H_i from the dense rows: the two cycle rows of device i are P_i + z_i <= C and Q_i - z_i <= C over the
        # integer columns; the least C of device i alone is max(P_i, (P_i + Q_i) / 2)
        A, b = p["A_ub"], p["b_ub"]
        xi = np.concatenate([np.rint(xo[:6 * M]), np.zeros(M + 1)])
        H = np.empty(M)
        for i in range(M):
            rows = np.flatnonzero(A[:, 6 * M + i])
            P = next(float(A[r] @ xi - b[r]) for r in rows if A[r, 6 * M + i] > 0)
            Q = next(float(A[r] @ xi - b[r]) for r in rows if A[r, 6 * M + i] < 0)
            H[i] = max(P, 0.5 * (P + Q))
        assert H.max() > 0.0
        top = np.flatnonzero(H >= H.max() - 1e-12 * abs(H.max()))
        assert e.bottleneck in top, (case, k, e.bottleneck, top)
        assert pc.close(e.cycle, float(H.max())), (case, k, e.cycle, H.max())
        count += 1
    assert count >= 400


def test_numpy_plan_evaluation_of_neighbours(tables):
    """Six neighbours of every kv 4bit optimum (drawn as tests/golden/gen_plans.py draws them, fixed seed)
    against HiGHS with the w and n columns fixed: status, objective within 1e-9. At least one slack_over_bound
    rejection (they come from pc.NEIGHBOUR_EXTRA: see there), and both classes above 15 %."""
    model = pc.our_model()
    nb = [q for q in pc.neighbour_plans() if q[2] != "optimum"]
    feas = slack = 0
    for case, k, kind, w, n in nb:
        e = pl.evaluate_plan_np(tables[case], model, 0, k, w, n, 0.5)
        ok, obj = pc.price_fixed(case, k, w, n)
        assert e.feasible == ok, (case, k, kind, w, n, e.reason)
        if ok:
            feas += 1
            assert pc.close(e.obj_value, obj), (case, k, kind, e.obj_value, obj)
        else:
            assert e.reason != 0 and e.obj_value == np.inf and e.bottleneck == -1
            slack += bool(e.reason & pl.REASON_SLACK)
    print(f"{len(nb)} neighbours: {feas} feasible, {len(nb) - feas} infeasible, {slack} slack_over_bound")
    assert len(nb) == 6 * sum(1 for q in pc.neighbour_plans() if q[2] == "optimum") >= 6 * 320
    assert slack >= 1
    assert feas > 0.15 * len(nb) and len(nb) - feas > 0.15 * len(nb), (feas, len(nb))


@pytest.mark.parametrize("M,scale,seed", [(3, pc.S16, 1), (16, pc.S64, 2), (64, pc.S64, 3)])
def test_lowering_matches_oracle_under_pressure(M, scale, seed):
    devs = pc.devices(seed, M, scale)
    for kv in ("4bit", "fp16"):
        fl = lower_fleet(devs, pc.our_model(), kv)
        for k in (1, 2, 5):
            _check(fl, k, mo.lower_dense(devs, pc.our_model(), k, pc.kv_factor(kv)))


# ------------------------------------------------------------------ the reference's recorded results
@pytest.fixture(scope="module")
def golden():
    return load_json("pressure.json")


def test_pressure_golden_is_data_in_the_regime(golden):
    fleets = golden["fleets"]
    assert (golden["kv_bits"], golden["mip_gap"]) == ("4bit", 1e-4)
    want = [(M, [sc.numerator, sc.denominator], s) for (M, sc) in pc.CLASSES for s in pc.golden_seeds(M)]
    assert [(f["M"], f["scale"], f["seed"]) for f in fleets] == want
    inst = []
    for f in fleets:
        assert set(f) == {"M", "scale", "seed", "result", "error", "per_k"}
        assert f["error"] is None and f["result"] is not None
        assert [r["k"] for r in f["per_k"]] == list(pc.KS)
        inst += [((f["M"], Fraction(*f["scale"]), f["seed"], "4bit"), r["k"]) for r in f["per_k"] if r["success"]]
    sh = pc.shares(inst)
    for key, floor in pc.FLOORS.items():
        assert sh[key] >= floor * sh["feasible"], (key, sh)


@pytest.mark.parametrize("solver", ["exact", "highs"])
def test_oracle_reproduces_the_recorded_pressure_results(golden, solver):
    for f in golden["fleets"]:
        assert pc.golden_mismatch(f, solver) is None, (f["M"], f["scale"], f["seed"], pc.golden_mismatch(f, solver))
