"""The structure of tests/deep_cases.py by the oracles alone (tests/golden/deep.json): the lists are what
test_gpu_deep.py needs them to be. Conditions, not measurements; tests/golden/gen_deep.py runs deep_conditions
before it writes."""

import pytest

from distilp_amd.solver import change as ch

from . import change_cases as cc
from . import deep_cases as dc


def _steps(vals):
    """(strictly improving steps, steps) between consecutive recorded points."""
    better = sum((a is None and b is not None) or (a is not None and b is not None and b < a)
                 for a, b in zip(vals, vals[1:]))
    return better, len(vals) - 1


def deep_conditions(gold):
    """Assert every condition on the recorded answers; the lines of the case table."""
    lines = []
    moving = [n for n in dc.WIDE if n not in dc.FLAT]
    # wide budget: every case has an improving step, two thirds of all steps improve
    tot = [0, 0]
    for n in moving:
        b, s = _steps([gold["wide"][n]["budget"]["obj"][str(p)] for p in dc.PS_W])
        assert b >= 1, n
        tot[0] += b
        tot[1] += s
    assert 3 * tot[0] >= 2 * tot[1], tot
    lines.append(f"wide budget: {len(dc.WIDE)} cases, {tot[0]} of {tot[1]} steps of the k = 2 parents improve")
    # wide change: per parent a list that ends better than it starts, and an optimum that releases a layer
    n_lists = 0
    for n in moving:
        lists = gold["wide"][n]["lists"]
        n_lists += len(lists)
        ends = [g["obj"][str(dc.PS_W[-1])] is not None and
                (g["obj"]["0"] is None or g["obj"][str(dc.PS_W[-1])] < g["obj"]["0"]) for g in lists.values()]
        rel = [r for g in lists.values() for r in g["released"].values() if r]
        assert any(ends) and rel, (n, ends, rel)
        lines.append(f"wide change {n}: {len(lists)} lists, {sum(ends)} end better than point 0, "
                     f"{len(rel)} recorded optima release a layer")
    # the constructed parents: the recorded optimum's cycle time belongs to a lane >= 32 and lies above every H
    # of lanes 0 .. 31, so no threshold drawn from those lanes alone admits it. Every budget point; the first
    # three points of at least four change lists.
    for n in [n for n in dc.WIDE if dc.WIDE[n][0] == "f"]:
        def pinned(sc):
            return [p for p in dc.PS_W if sc["lane"][str(p)] >= 32 and sc["cycle"][str(p)] > sc["fast_top"]]

        g = gold["wide"][n]
        assert pinned(g["budget"]["scan"]) == list(dc.PS_W), n
        held = {ln: pinned(r["scan"]) for ln, r in g["lists"].items()}
        assert sum(v[:3] == [0, 1, 2] for v in held.values()) >= 4, (n, held)
        lines.append(f"threshold scan {n}: {len(dc.PS_W)} budget points and "
                     f"{sum(len(v) for v in held.values())} change points of {len(held)} lists need a threshold of "
                     f"lanes 32 .. 63")
    # the W = M parents: one plan, nothing to release
    for n in dc.FLAT:
        g = gold["wide"][n]
        assert set(g["w"]) == {1} and len(set(g["budget"]["obj"].values())) == 1, n
        for ln, rec in g["lists"].items():
            assert len(set(rec["obj"].values())) == 1 and rec["obj"]["0"] is not None, (n, ln)
            assert set(rec["released"].values()) == {0}, (n, ln)
        n_lists += len(g["lists"])
    # deep: the byte edge
    cases = dc.deep_cases()
    assert set(cases) == set(gold["deep"])
    at254 = [n for n, e in cases.items()
             if e["entry"] == 254 and all(v is not None for v in gold["deep"][n]["obj"].values())]
    at253 = [n for n, e in cases.items() if e["entry"] == 253]
    assert len(at254) >= 3 and at253, (at254, at253)
    assert {(e["P"], e["D"]) for e in cases.values()} >= {(0, 254), (1, 252), (27, 200)}
    top_w = max(v for g in gold["deep"].values() for v in g["max_w"].values() if v is not None)
    idx = sorted(v for g in gold["deep"].values() for v in g["max_index"].values() if v is not None)
    assert top_w > 255 and sum(v > 127 for v in idx) >= 1 and sum(v > 200 for v in idx) >= 1, (top_w, idx)
    assert any(a > 255 for e in cases.values() for a in e["w0"])
    lines.append(f"deep change: {len(cases)} lists, {len(at254)} feasible at 2 P + D = 254, {len(at253)} at 253, "
                 f"largest recorded w_i {top_w}, {sum(v > 127 for v in idx)} recorded window indices above 127, "
                 f"{sum(v > 200 for v in idx)} above 200")
    for a, b in dc.PAIRS.values():
        assert cases[a]["D"] == max(cases[a]["D"], cases[b]["D"]) > cases[b]["D"] == 0
        assert (cases[a]["L"], cases[a]["k"], cases[a]["P"]) == (cases[b]["L"], cases[b]["k"], cases[b]["P"])
    assert set(dc.deep_budget_cases()) == set(gold["deep_budget"])
    for n, e in dc.deep_budget_cases().items():
        assert max(e["w0"]) > 255 and e["P"] in (62, 63)
        b, _ = _steps(list(gold["deep_budget"][n]["obj"].values()))
        assert b >= 1, n
    lines.append(f"deep budget: {len(gold['deep_budget'])} cases at P = 62 and 63")
    # at most one recorded point in ten is infeasible
    pts = [v for g in gold["wide"].values() for v in g["budget"]["obj"].values()]
    pts += [v for g in gold["wide"].values() for r in g["lists"].values() for v in r["obj"].values()]
    pts += [v for sec in ("deep", "deep_budget") for g in gold[sec].values() for v in g["obj"].values()]
    nulls = sum(v is None for v in pts)
    assert 10 * nulls <= len(pts), (nulls, len(pts))
    lines.append(f"recorded points: {len(pts)}, {nulls} without a plan; wide change lists in all: {n_lists}")
    for case in dc.SUBSETS:
        bf = gold["subsets"][dc.subset_id(case)]
        assert len(bf) == case[1] + 1 and all(b[0] is not None for b in bf)
    lines.append(f"subsets: {len(dc.SUBSETS)} fleets")
    return lines


def test_the_recorded_lists_meet_their_conditions():
    for line in deep_conditions(dc.golden()):
        print(line)


def test_the_golden_file_describes_the_case_lists(llama_online_model):
    """The incumbents, w0 and D of the file are the ones deep_cases builds now; the cheapest answers are
    re-derived (a one-device list has one plan)."""
    model, gold = llama_online_model, dc.golden()
    assert set(gold["wide"]) == set(dc.WIDE)
    for name, (kind, M, s, L, k) in dc.WIDE.items():
        g = gold["wide"][name]
        assert sum(g["w"]) == L // k and len(g["w"]) == M and min(g["w"]) >= 1
        lists = dc.wide_lists(name, dc.wide_devices(name), g["w"])
        assert set(lists) == set(g["lists"])
        for ln, (_, keep, w0) in lists.items():
            assert (g["lists"][ln]["w0"], g["lists"][ln]["D"]) == (w0, L // k - sum(w0)), (name, ln)
    name = "w48"  # one incumbent re-solved: the exact optimum of seed s + 100
    assert dc.wide_incumbent(model, name) == gold["wide"][name]["w"]
    name = "f64"  # the constructed parent: its order, its incumbent and point 0's witness re-derived
    kind, M, s, L, k = dc.WIDE[name]
    devs, g = dc.wide_devices(name), gold["wide"][name]
    assert sorted(d.name for d in devs) == sorted(d.name for d in dc.bc.devices(M, s))
    assert dc.wide_incumbent(model, name) == g["w"]
    c, lane, top = dc.scan_witness(dc.model_at(model, L), devs, k, g["w"], max(dc.PS_W), g["w"])
    sc = g["budget"]["scan"]
    assert lane == sc["lane"]["0"] >= 32 and abs(c - sc["cycle"]["0"]) <= 1e-12 and abs(top - sc["fast_top"]) <= 1e-12
    assert c > top
    for name, e in dc.deep_cases().items():
        g = gold["deep"][name]
        assert (g["w0"], g["D"], sorted(g["obj"])) == (e["w0"], e["D"], sorted(str(p) for p in e["ps"])), name
        if len(e["idx"]) == 1:
            ans = dc.deep_answer(model, e)
            assert all(abs(ans[p] - g["obj"][str(p)]) <= 1e-9 * max(1.0, abs(ans[p])) for p in e["ps"]), name
            assert g["max_w"]["0"] == e["L"] // e["k"] and g["max_index"]["0"] == e["D"] == 254


def test_the_gate_admits_the_edge_and_nothing_past_it():
    """change.check_gate on the shapes alone: every deep case is inside, every rejected case outside."""
    for name, e in dc.deep_cases().items():
        m = len(e["idx"])
        ch.check_gate(m, m, e["P"], e["D"], e["k"])
        assert cc.gate_p(ch, m, e["D"], e["k"]) >= e["P"], name
    for name, e in dc.rejected_cases().items():
        m = len(e["idx"])
        with pytest.raises(ValueError, match=e["error"]):
            ch.check_gate(m, m, e["P"], e["D"], e["k"])
        assert e["entry"] == (255 if e["error"] == "254" else 254), name
    # what the gate's arithmetic says at the edge
    assert cc.gate_p(ch, 16, 252, 1) == 1 and cc.gate_p(ch, 16, 254, 1) == 0
    assert cc.gate_p(ch, 3, 200, 1) == 27 and cc.gate_p(ch, 16, 200, 1) == 17
    assert cc.gate_p(ch, 64, 254, 1) == 0 and cc.gate_p(ch, 64, 254, 2) == -1
