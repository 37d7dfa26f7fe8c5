"""Generate tests/golden/deep.json: the recorded answers of tests/deep_cases.py.

Run:  python tests/golden/gen_deep.py [section ...]     (needs the built oracle, `make -C oracle`)

About 4 minutes on one CPU core (printed per section at the end); with section names (wide, deep, deep_budget,
subsets) only those are recomputed and merged into the file.

Both oracles are this repository's own (tests/budget_cases.py, tests/change_cases.py). Recorded results only, no
plans:

  "wide": {parent: {"w": the stale incumbent,
                    "budget": {"obj": {p: obj_value or null}},
                    "lists": {list: {"w0", "D", "obj": {p: ...}, "released": {p: released layers of oracle (b)'s w},
                                     "free_released", "free_unique"}}}}
          (a kind "f" parent also "scan": {"cycle": {p: the recorded optimum's cycle time}, "lane": {p: its
          bottleneck lane}, "fast_top": the largest H of lanes 0 .. 31 in their windows}, for its budget and lists)
  "deep": {case: {"w0", "D", "obj": {p: ...}, "max_w": {p: the largest w_i of oracle (b)'s w},
                  "max_index": {p: the largest window index w_i - max(1, w0_i - P) of it}}}
  "deep_budget": {case: {"w0", "obj": {p: ...}}}
  "subsets": {case: [[best obj or null, dropped or null, runner-up obj or null] per d]}

The generator STOPS where the two oracles disagree beyond 1e-9 relative and where the lists miss what
tests/test_deep.py asks of them (it runs the same conditions, deep_conditions, before it writes)."""

from __future__ import annotations

import json
import math
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))


def _model():
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.synth import load_model_dict

    return ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()


def _oracle_b_w(model, devs, k, w0, ps):
    """{p: oracle (b)'s w or None}: what the recorded optimum does, not only what it costs."""
    from tests import budget_cases as bu
    from tests import change_cases as cc

    prob = bu.problem(model, devs, k)
    return {p: cc.highs_change(prob, w0, p)[1] for p in ps}


def _witness(model, devs, k, w0, ws):
    """{"cycle": {p: ...}, "lane": {p: ...}, "fast_top": ...} of oracle (b)'s plans ws (deep_cases.scan_witness)."""
    from tests import deep_cases as dc

    out = {"cycle": {}, "lane": {}, "fast_top": None}
    for p, w in ws.items():
        c, lane, top = dc.scan_witness(model, devs, k, w0, max(dc.PS_W), w)
        out["cycle"][str(p)], out["lane"][str(p)], out["fast_top"] = c, lane, top
    return out


def wide(model):
    from tests import budget_cases as bu
    from tests import change_cases as cc
    from tests import deep_cases as dc

    out = {}
    for name, (kind, M, s, L, k) in dc.WIDE.items():
        m, devs = dc.model_at(model, L), dc.wide_devices(name)
        w = dc.wide_incumbent(model, name)
        prob = bu.problem(m, devs, k)
        pin, objs = bu.Pinned(prob), {}
        for p in dc.PS_W:
            b, wb = bu.highs_budget(prob, w, p)
            e = None
            if b is not None:
                e = pin(wb)
                assert e is not None and dc.bc.rel(b, e) <= 1e-9, (name, p, b, e)
                assert sum(wb) == prob["W"] and sum(max(0, x - y) for x, y in zip(wb, w)) <= p
            objs[str(p)] = e
        rec = {"w": w, "budget": {"obj": objs}, "lists": {}}
        if kind == "f":
            rec["budget"]["scan"] = _witness(m, devs, k, w, {p: bu.highs_budget(prob, w, p)[1] for p in dc.PS_W})
        print(name, "budget", list(objs.values()), flush=True)
        for ln, (parent, keep, w0) in dc.wide_lists(name, devs, w).items():
            listed = [parent[j] for j in keep]
            ans = cc.answer(m, listed, k, w0, dc.PS_W, "b", tag=(name, ln))
            ws = _oracle_b_w(m, listed, k, w0, dc.PS_W)
            fr, uniq = cc.free_optimum(m, listed, k, w0)
            rec["lists"][ln] = {"w0": w0, "D": L // k - sum(w0), "obj": {str(p): ans[p] for p in dc.PS_W},
                                "released": {str(p): None if ws[p] is None else cc.released(ws[p], w0)
                                             for p in dc.PS_W},
                                "free_released": fr, "free_unique": uniq}
            if kind == "f":
                rec["lists"][ln]["scan"] = _witness(m, listed, k, w0, ws)
            print(name, ln, rec["lists"][ln]["D"], list(ans.values()), list(rec["lists"][ln]["released"].values()),
                  fr, flush=True)
        out[name] = rec
    return out


def deep(model):
    from tests import deep_cases as dc

    out = {}
    for name, e in dc.deep_cases().items():
        t = time.time()
        ans = dc.deep_answer(model, e)
        ws = _oracle_b_w(dc.model_at(model, e["L"]), [e["devs"][j] for j in e["idx"]], e["k"], e["w0"], e["ps"])
        lo = [max(1, a - e["P"]) for a in e["w0"]]
        out[name] = {"w0": e["w0"], "D": e["D"], "obj": {str(p): ans[p] for p in e["ps"]},
                     "max_w": {str(p): None if ws[p] is None else max(ws[p]) for p in e["ps"]},
                     "max_index": {str(p): None if ws[p] is None else max(a - b for a, b in zip(ws[p], lo))
                                   for p in e["ps"]}}
        print(name, out[name], f"{time.time() - t:.1f} s", flush=True)
    return out


def deep_budget(model):
    from tests import deep_cases as dc

    out = {}
    for name, e in dc.deep_budget_cases().items():
        ans = dc.deep_budget_answer(model, e)
        out[name] = {"w0": e["w0"], "obj": {str(p): v for p, v in ans.items()}}
        print(name, out[name], flush=True)
    return out


def subsets(model):
    from tests import deep_cases as dc
    from tests import subsets_cases as sc

    out = {}
    for case in dc.SUBSETS:
        bf = sc.brute_force_of(*case)
        out[dc.subset_id(case)] = [[None if b == math.inf else b, None if g is None else list(g),
                                    None if r == math.inf else r] for b, g, r in bf]
        print(dc.subset_id(case), out[dc.subset_id(case)], flush=True)
    return out


def main():
    from tests.test_deep import deep_conditions

    model = _model()
    path = HERE / "deep.json"
    sections = {"wide": wide, "deep": deep, "deep_budget": deep_budget, "subsets": subsets}
    todo = sys.argv[1:] or list(sections)
    out = json.loads(path.read_text()) if path.exists() and sys.argv[1:] else {}
    took = {}
    for name in todo:
        t = time.time()
        out[name] = sections[name](model)
        took[name] = time.time() - t
    if set(out) == set(sections):
        for line in deep_conditions(out):
            print(line)
    path.write_text(json.dumps({n: out[n] for n in sections if n in out}, indent=1) + "\n")
    print("running time:", ", ".join(f"{n} {t:.0f} s" for n, t in took.items()), f"; total {sum(took.values()):.0f} s")


if __name__ == "__main__":
    main()
