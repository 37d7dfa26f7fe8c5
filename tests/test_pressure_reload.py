"""The reload ladder without a GPU: boxes.reload_caps against exact rational arithmetic (fractions.Fraction of the
same m / s_disk quotients) on fleets whose quotients collide across devices and on an s_disk for which m * (1 / s) and
m / s differ in the last bit, and the condition the pressured reload cases are chosen for."""

from fractions import Fraction

import numpy as np
import pytest

from distilp_amd.solver.boxes import reload_caps

from . import pressure_reload_cases as rc


def exact_caps(w0, s_disk, W):
    """(t, caps) by rational arithmetic: t = 0 and the distinct m / s_i in ascending order, caps[j][i] the number of
    m with m / s_i <= t[j]."""
    M = len(w0)
    quot = [[Fraction(m) / Fraction(s_disk[i]) for m in range(1, max(0, W - (M - 1) - w0[i]) + 1)] for i in range(M)]
    t = [Fraction(0)] + sorted({q for qs in quot for q in qs})
    return t, [[sum(q <= v for q in qs) for qs in quot] for v in t]


def check(w0, s_disk, W):
    t, caps = reload_caps(w0, s_disk, W, max_points=1 << 20)
    te, ce = exact_caps(w0, s_disk, W)
    fl = [float(v) for v in te]  # correctly rounded, as the one FP64 division of m / s is
    assert all(a < b for a, b in zip(fl, fl[1:]))  # no two distinct quotients round onto one double here
    assert t.tolist() == fl and caps.tolist() == ce
    return t, caps


def test_two_devices_whose_quotients_collide_are_one_point():
    """2 / 3.0 and 1 / 1.5 are the same rational: one breakpoint, and both devices' caps step at it."""
    w0, s, W = [3, 2, 4], [3.0, 1.5, 7.0], 20
    assert 2 / s[0] == 1 / s[1]
    t, caps = check(w0, s, W)
    j = t.tolist().index(2 / 3.0)
    assert (caps[j] - caps[j - 1]).tolist()[:2] == [1, 1]
    n_quot = sum(W - 2 - w for w in w0)
    assert len(t) < 1 + n_quot  # collisions merged


def test_an_s_disk_whose_reciprocal_rounds_differently():
    """s = 49: 49 * (1 / 49) is 1 - 2^-53 ... not 49 / 49; a cap counted on m * (1 / s) would miss the breakpoint of
    the device with s = 1 at t = 1. 24.5 collides with it (2 / 49 = 1 / 24.5)."""
    s = [49.0, 24.5, 1.0]
    bad = [m for m in range(1, 78) if m * (1.0 / s[0]) != m / s[0]]
    assert 49 in bad
    t, caps = check([1, 1, 1], s, 80)
    j = t.tolist().index(1.0)
    assert caps[j].tolist() == [49, 24, 1]
    assert caps[t.tolist().index(2 / 49.0)].tolist() == [2, 1, 0]


@pytest.mark.parametrize("fleet", rc.FLEETS)
def test_the_pressured_ladders_equal_rational_arithmetic(fleet):
    w0, s = rc.incumbent(fleet), [float(d.s_disk) for d in rc.devices(fleet)]
    t, caps = check(w0, s, 80 // fleet[2])
    ct, cc = rc.ladder(fleet)
    assert len(ct) == rc.MAX_POINTS and np.array_equal(ct, t[:rc.MAX_POINTS])
    assert np.array_equal(cc, caps[:rc.MAX_POINTS])
    assert not cc[0].any() and (np.diff(cc, axis=0) >= 0).all()


def test_some_ladder_has_consecutive_optima_that_differ_in_a_slack_or_t_column():
    steps = {f: rc.slack_steps(f) for f in rc.FLEETS}
    assert any(steps.values()), steps
    for f in rc.FLEETS:
        fr = rc.frontier(f)
        assert fr[0] is not None and all(b <= a for a, b in zip(fr, fr[1:]))
        M = f[0]
        assert np.rint(rc.raw_points(f)[0][1][:M]).tolist() == rc.incumbent(f)  # point 0: w pinned
