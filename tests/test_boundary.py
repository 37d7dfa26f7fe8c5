"""Capacity rows a few bytes short of a whole number of layers (tests/golden/boundary.json, see tests/boundary.py):
the exact oracle, with the slack rule's tolerance SLACK_EPS = 1e-6 layers, reproduces the reference on every
kind of capacity row (halda_p_solver.py:226-277), inside and outside the window 1e-9 b' < delta <= 0.9e-6 b' in
which the reference's HiGHS takes the integer slack delta / b' as 0. CPU only."""

import collections

import pytest

from oracle import milp_oracle as mo

from . import boundary as bd


@pytest.fixture(scope="module")
def exact_runs():
    """[(group, case, best, per_k)] of the exact oracle's k-sweep on every case (computed once)."""
    out = []
    for g, c in bd.all_cases():
        _, model = bd.base_fleet(g["fleet"])
        best, per_k = mo.halda_solve_oracle(bd.devices(g, c), model, k_candidates=g["ks"], mip_gap=1e-4,
                                            kv_bits=g["kv_bits"], solver="exact")
        out.append((g, c, best, per_k))
    return out


def _tag(g, c):
    return (g["fleet"], g["kv_bits"], g["device"], g["row"], g["j"], c["delta"])


def test_exact_oracle_reproduces_the_reference(exact_runs):
    """(k, w, n, sets) and every per-k status / w / n equal the golden's, obj_value within 1e-9 of the
    reference's objective re-evaluated at its rounded integer columns; reference_failure cases against the
    presolve-off record, reference_unstable cases against the HiGHS answer their `match` names, and the tied
    ones among them by objective."""
    counts = collections.Counter()
    for g, c, best, per_k in exact_runs:
        counts[bd.klass(c)] += 1
        want = bd.expected(g, c)
        if want is None:
            bd.check_tied(per_k, g, c, _tag(g, c))
            continue
        res, want_k = want
        bd.check_per_k(per_k, want_k, _tag(g, c))
        assert (best["k"], best["w"], best["n"], best["sets"]) == (res["k"], res["w"], res["n"], g["sets"]), _tag(g, c)
    assert counts["ok"] and counts["reference_failure"] and counts["reference_unstable"], counts


def test_highs_still_gives_the_golden_answers():
    """The fixture describes this HiGHS: the oracle's own HiGHS call (presolve on, as the reference calls it)
    gives the golden's per-k status / w / n on a sample of ~20 cases, failures and unstable cases included."""
    cases = bd.all_cases()
    ok = [t for t in cases if bd.klass(t[1]) == "ok"]
    sample = ok[::max(1, len(ok) // 14)][:14]
    sample += [t for t in cases if bd.klass(t[1]) == "reference_failure"][:4]
    sample += [t for t in cases if bd.klass(t[1]) == "reference_unstable"][:2]
    assert len(sample) >= 18
    for g, c in sample:
        _, model = bd.base_fleet(g["fleet"])
        _, per_k = mo.halda_solve_oracle(bd.devices(g, c), model, k_candidates=g["ks"], mip_gap=1e-4,
                                         kv_bits=g["kv_bits"], solver="highs")
        for a, b in zip(per_k, bd.unpack(g, c)):
            assert a["success"] == b["success"], (_tag(g, c), b["k"])
            if b["success"]:
                assert (a["w"], a["n"]) == (b["w"], b["n"]), (_tag(g, c), b["k"])


def _answer(g, c):
    """(k, w, n) the reference stands for on case c: its own (ok) or its presolve-off answer (reference_failure);
    None for a reference_unstable case, where presolve on and off disagree."""
    if bd.klass(c) == "reference_unstable":
        return None
    want = bd.expected(g, c)
    return (want[0]["k"], want[0]["w"], want[0]["n"])


def test_file_structure():
    """Every row kind is present, Metal VRAM on a head and on a non-head device; every group's boundary is
    binding (the reference at -10 B differs from the reference at 10^4 B); the classes that are not plain
    reference answers are capped; and the window exists in the data alone: where every row the edited field
    feeds is short by <= 0.9 T the reference answers as at -10 B, where every one is short by >= 1.1 T as at
    10^4 B."""
    G = bd.golden()
    cases = bd.all_cases()
    kinds = collections.Counter(g["row"] for g, _ in cases)
    assert set(kinds) == set(bd.KINDS), kinds
    assert {g["head"] for g in G["groups"] if g["row"] == "metal_vram"} == {True, False}  # rhs carries b_out * head
    assert any(g["row"] == "M2" and "metal_vram" in g["rows_moved"] for g in G["groups"])
    assert any(g["row"] == "M3_android" and c["edits"]["d_swap_avail"] > 0 for g, c in cases)
    assert {g["kv_bits"] for g in G["groups"]} == {"4bit", "fp16"}
    # caps: the issue's 10 % on reference_failure; reference_unstable (HiGHS against itself) may not grow past a
    # fifth of the file, nor its tied cases, compared by objective only, past 5 %, when the file is regenerated
    n_fail = sum(bd.klass(c) == "reference_failure" for _, c in cases)
    n_unst = sum(bd.klass(c) == "reference_unstable" for _, c in cases)
    n_tied = sum(bd.klass(c) == "reference_unstable" and c["match"] is None for _, c in cases)
    assert n_fail <= 0.10 * len(cases), (n_fail, len(cases))
    assert n_unst <= 0.20 * len(cases) and n_tied <= 0.05 * len(cases), (n_unst, n_tied, len(cases))
    in_ok = collections.Counter()
    for g in G["groups"]:
        tag = (g["fleet"], g["kv_bits"], g["device"], g["row"], g["j"])
        T = g["T"]
        assert abs(T - 1e-6 * g["b_prime"]) <= 1e-12 * T
        by_target = {c["delta_target"]: c for c in g["cases"]}
        lo, hi = by_target[-10.0], by_target[10000.0]
        assert bd.klass(lo) == bd.klass(hi) == "ok", tag
        assert _answer(g, lo) != _answer(g, hi), tag
        for c in g["cases"]:
            assert not (0.9 * T < c["delta"] < 1.1 * T), (tag, c["delta"])  # the edge itself is not pinned
            assert abs(c["delta"] - (g["j"] * g["b_prime"] - c["rhs"])) <= 2e-6
            assert abs(c["delta"] - c["delta_target"]) <= 1.001, (tag, c["delta"], c["delta_target"])
            assert set(c.get("delta_rows", {})) == set(g["rows_moved"]) - {g["row"]}, tag
            ans = _answer(g, c)
            if ans is None:
                # unstable: HiGHS with and without presolve disagree (our code takes no part in the label)
                on, off = bd.unpack(g, c), bd.unpack(g, c, "a_nopre")
                assert [(r["status"], r.get("w"), r.get("n"), r.get("obj_value_rint")) for r in on] != [
                    (r["status"], r.get("w"), r.get("n"), r.get("obj_value_rint")) for r in off], tag
                continue
            # a head Metal device's M2 row is b_in / V further short than its VRAM row: both rows count
            deltas = [c["delta"]] + list(c.get("delta_rows", {}).values())
            if max(deltas) <= 0.9 * T:
                assert ans == _answer(g, lo), (tag, deltas)
                in_ok[g["row"]] += bd.in_window(g, c)
            elif min(deltas) >= 1.1 * T:
                assert ans == _answer(g, hi), (tag, deltas)
    assert set(in_ok) == set(bd.KINDS) and min(in_ok.values()) >= 4, in_ok  # stable in-window cases of every kind


def test_old_tolerance_misses_the_window():
    """Regression guard: with the former eps = 1e-9 layers the exact solver disagrees with the golden on
    in-window cases of every row kind, so the fixture pins the rule."""
    missed = collections.Counter()
    for g, c in bd.all_cases():
        if bd.klass(c) != "ok" or not bd.in_window(g, c):
            continue
        _, model = bd.base_fleet(g["fleet"])
        _, per_k = mo.halda_solve_oracle(bd.devices(g, c), model, k_candidates=g["ks"], mip_gap=1e-4,
                                         kv_bits=g["kv_bits"], solver="exact", eps=1e-9)
        want = bd.unpack(g, c)
        if any(a["success"] != b["success"] or (b["success"] and (a["w"], a["n"]) != (b["w"], b["n"]))
               for a, b in zip(per_k, want)):
            missed[g["row"]] += 1
    assert set(missed) == set(bd.KINDS), missed
