"""Boundary goldens (tests/golden/boundary.json, written by `python tests/golden/gen_golden.py boundary`):
fleets whose one capacity row is delta bytes short of a whole number j of layers (rhs = j b' - delta),
solved by the reference. Shared by test_boundary.py (CPU) and test_gpu_boundary.py.

File layout: "fleets" names the base fleets (a profile folder, or synth_fleet(seed, M) with `mods` set on
some devices); each group is one (fleet, kv_bits, device, row kind, j) with its k list, the reference's
sets, b' and T = 1e-6 b', and the distinct per-k `answers` of its cases (parallel arrays over the group's ks:
HiGHS status, w, n, lin_rint = c.x at the rounded integer columns); each case of a group sets `edits` on the
group's device and records the achieved rhs / delta, the reference's result (k, obj_value), its answer by index
("a"; presolve off: "a_nopre"), the objective constant (obj_value_rint = lin_rint + const), `excess` (HiGHS's
own obj_value minus obj_value_rint, where not 0) and a class (absent: ok):
  ok                  HiGHS gives the same per-k answers with and without presolve;
  reference_failure   presolve changes an answer, |delta| <= 2 B, and without presolve HiGHS agrees with
                      the exact solver: compared against the presolve-off record ("nopre", "result_nopre");
  reference_unstable  presolve changes an answer anywhere else (HiGHS against itself);
                      `match` names the HiGHS answer that is the exact optimum under the slack rule and is
                      compared in full ("a_nopre" or "a"), or is null (a tie, or both HiGHS answers above the optimum): never worse.
Cases whose edited field feeds a second row record that row's own achieved delta in `delta_rows`.
"""

import copy
import glob
import json
from functools import lru_cache

from .conftest import REPO, load_json

OBJ_REL = 1e-9
KINDS = ("M1", "M2", "M3", "M3_android", "cuda_vram", "metal_vram")


@lru_cache(maxsize=None)
def golden():
    return load_json("boundary.json")


@lru_cache(maxsize=None)
def base_fleet(name):
    """(device dicts, model) of a base fleet of the golden file."""
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.synth import load_model_dict, synth_fleet

    f = golden()["fleets"][name]
    if "folder" in f:
        base = REPO / "test" / "profiles" / f["folder"]
        files = sorted(p for p in glob.glob(str(base / "*.json")) if not p.endswith("model_profile.json"))
        dicts = [json.loads(open(p).read()) for p in files]
        dicts[0]["is_head"] = True  # as the profile-folder loader marks it
        model = ModelProfileSplit.model_validate(json.loads((base / "model_profile.json").read_text()))
        return dicts, model.to_model_profile()
    dicts = synth_fleet(f["seed"], f["M"])
    for m in f["mods"]:
        dicts[m["dev"]].update(m["set"])
    return dicts, ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()


def devices(g, c):
    """The DeviceProfiles of case c of group g."""
    from distilp_amd.common import DeviceProfile

    dicts, _ = base_fleet(g["fleet"])
    dicts = copy.deepcopy(dicts)
    dicts[g["device"]].update(c["edits"])
    return [DeviceProfile.model_validate(d) for d in dicts]


def unpack(g, c, which="a"):
    """Per-k dicts (k, status, success, w, n, obj_value_rint, and for the presolve-on answer obj_value) of case
    c's presolve-on answer ("a") or presolve-off answer ("a_nopre")."""
    rec = g["answers"][c[which]]
    out = []
    for j, k in enumerate(g["ks"]):
        r = {"k": k, "status": rec["status"][j], "success": rec["status"][j] == 0}
        if r["success"]:
            r["w"], r["n"] = rec["w"][j], rec["n"][j]
            r["obj_value_rint"] = rec["lin_rint"][j] + c["const"]
            if which == "a":
                r["obj_value"] = r["obj_value_rint"] + c.get("excess", {}).get(str(j), 0.0)
        out.append(r)
    return out


def klass(c):
    return c.get("class", "ok")


def _result(per_k, res):
    if res is None:
        return None
    at = next(r for r in per_k if r["k"] == res["k"])
    return {"k": res["k"], "w": at["w"], "n": at["n"], "obj_value": res["obj_value"]}


def expected(g, c):
    """(result, per-k dicts) a solver has to reproduce for case c: the reference's own answers (ok); its
    presolve-off answers (reference_failure, and reference_unstable cases whose `match` is "a_nopre"); its
    presolve-on answers (reference_unstable, match "a"). None for a reference_unstable case without a match:
    neither HiGHS answer is the unique optimum, see check_tied."""
    which = {"ok": "a", "reference_failure": "a_nopre"}.get(klass(c), c.get("match"))
    if which is None:
        return None
    per_k = unpack(g, c, which)
    return _result(per_k, c["result"] if which == "a" else c["result_nopre"]), per_k


def all_cases():
    """[(group, case)] of the file, in file order."""
    return [(g, c) for g in golden()["groups"] for c in g["cases"]]


def in_window(g, c):
    """The row is short by more than 1e-9 layers (the old rule adds a slack layer) and by at most
    0.9e-6 layers (the reference does not)."""
    return 1e-9 * g["b_prime"] < c["delta"] <= 0.9 * g["T"]


def obj_close(a, b):
    return abs(a - b) <= OBJ_REL * max(1.0, abs(b))


def check_per_k(got, want, tag):
    """got: per-k dicts (success, w, n, obj_value) of a solver; want: expected(...)[1]."""
    assert len(got) == len(want), tag
    for a, b in zip(got, want):
        assert a["success"] == b["success"], (tag, b["k"], a["success"], b["status"])
        if b["success"]:
            assert (a["w"], a["n"]) == (b["w"], b["n"]), (tag, b["k"], a["w"], a["n"], b["w"], b["n"])
            assert obj_close(a["obj_value"], b["obj_value_rint"]), (tag, b["k"], a["obj_value"], b["obj_value_rint"])


def check_tied(got, g, c, tag):
    """reference_unstable without a match: HiGHS with and without presolve give different (w, n) and neither is
    the exact optimum's (a tie, or a HiGHS answer above the optimum, some by more than its mip gap). These cases
    lie in the window, every row the edited field feeds included, where both HiGHS points are feasible under
    the slack rule: wherever either run found a solution the solver has one that is no worse than the better
    of the two (to 1e-9)."""
    assert max([c["delta"]] + list(c.get("delta_rows", {}).values())) <= 0.9 * g["T"], tag
    for a, on, off in zip(got, unpack(g, c), unpack(g, c, "a_nopre")):
        found = [r["obj_value_rint"] for r in (on, off) if r["success"]]
        if found:
            assert a["success"], (tag, on["k"])
            assert a["obj_value"] <= min(found) + OBJ_REL * max(1.0, abs(min(found))), (
                tag, on["k"], a["obj_value"], min(found))


FIELDS = ("n_cols", "n_rows", "csr_off", "col_off", "row_off", "row_ptr", "col_idx", "val", "c", "col_lb", "col_ub",
          "row_lb", "row_ub", "integrality")


def settled_device_solve(ctx, batch, settled, dev, stream):
    """halda_solve_batch_device_settled on device copies of a host batch; the results as NumPy arrays."""
    import numpy as np
    import torch

    keep = {f: torch.from_numpy(np.ascontiguousarray(getattr(batch, f))).to(dev) for f in FIELDS}
    n = batch.n_inst
    out = {"status": torch.full((n,), 7, dtype=torch.int32, device=dev),
           "x": torch.full((batch.total_cols,), -3.0, dtype=torch.float64, device=dev),
           "obj_lin": torch.full((n,), -5.0, dtype=torch.float64, device=dev),
           "dual_bound": torch.full((n,), -5.0, dtype=torch.float64, device=dev),
           "gap": torch.full((n,), -5.0, dtype=torch.float64, device=dev),
           "nodes": torch.full((n,), -9, dtype=torch.int64, device=dev)}
    hint = torch.from_numpy(settled).to(dev)
    torch.cuda.synchronize(dev)
    ctx.solve_device({f: t.data_ptr() for f, t in keep.items()}, batch, {f: t.data_ptr() for f, t in out.items()},
                     stream=stream.cuda_stream, settled=hint.data_ptr())
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}
