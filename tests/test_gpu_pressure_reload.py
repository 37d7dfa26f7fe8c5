"""halda_reload_frontier on memory-pressured fleets (tests/pressure_reload_cases.py) against the exact oracle solved
inside every rung's w_max: under a w_max ladder a pressured device's slack and t change with every rung, where on the
unscaled fleets of test_gpu_boxes.py the points differ only in w."""

import pytest

from distilp_amd.solver import _libhalda as lh
from distilp_amd.solver import boxes as bx
from distilp_amd.solver import halda_reload_frontier

from . import pressure_cases as pc
from . import pressure_reload_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fleet", rc.FLEETS)
def test_reload_frontier_under_pressure_equals_the_oracle(fleet):
    model = pc.our_model()
    M, _, k, _ = fleet
    devs, w0 = rc.devices(fleet), rc.incumbent(fleet)
    sd = [float(d.s_disk) for d in devs]
    inc = (k, w0, [0] * M)
    pts = halda_reload_frontier(devs, model, inc, max_points=rc.MAX_POINTS, kv_bits="4bit")
    route = bx.last_boxes_route(lh.get_context(0))
    t, caps = rc.ladder(fleet)
    want = rc.frontier(fleet)
    group = float(k * int(model.b_layer))
    assert len(pts) == rc.MAX_POINTS == len(want)
    for j, (p, o) in enumerate(zip(pts, want)):
        tag = (fleet, j)
        assert p.caps == caps[j].tolist() and p.seconds == float(t[j]) * group, tag
        assert (p.plan is None) == (o is None), tag
        assert o is None or pc.close(p.obj_value, o), tag + (p.obj_value, o)
        assert p.gained == [max(0, a - b) for a, b in zip(p.plan.w, w0)], tag
        assert all(g <= c for g, c in zip(p.gained, p.caps)), tag
        assert p.seconds_used == max(g / s for g, s in zip(p.gained, sd)) * group <= p.seconds, tag
        assert sum(p.plan.w) == pc.L // k and p.plan.k == k, tag
    # point 0 is the pinned-w optimum
    assert pts[0].plan.w == w0 and pts[0].gained == [0] * M and pts[0].seconds_used == 0.0
    assert pc.close(pts[0].obj_value, rc.raw_points(fleet)[0][0])
    assert any(b < a for a, b in zip(want, want[1:]))  # the ladder improves on "w pinned"
    # without a cut the last point is the unbounded optimum at k
    full = halda_reload_frontier(devs, model, inc, max_points=4096, kv_bits="4bit")
    st = pc.exact(rc.case_of(fleet), k)[0]
    assert st == 0 and len(full) > rc.MAX_POINTS
    assert pc.close(full[-1].obj_value, pc.objective(rc.case_of(fleet), k)) and full[-1].regret == 0.0
    assert [p.obj_value for p in full[:rc.MAX_POINTS]] == [p.obj_value for p in pts]
    for p in full:
        assert all(g <= c for g, c in zip(p.gained, p.caps)) and p.seconds_used <= p.seconds and p.regret >= 0.0
    print(f"reload {fleet}: route {route} / {bx.last_boxes_route(lh.get_context(0))}, {len(full)} points uncut, "
          f"slack or t changes after points {rc.slack_steps(fleet)}")
