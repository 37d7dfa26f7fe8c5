"""Generate golden vectors from the REFERENCE implementation (this container only).

Run:  python tests/golden/gen_golden.py          (needs /root/reference; ~1-2 min)

The reference (distilp 0.1.6, /root/reference/src) is imported read-only via the
3.10 shim of SURVEY.md §8c (PEP 695 `type` aliases pre-registered), with
bytecode writing disabled. Its `scipy.optimize.milp` call site
(halda_p_solver.py:340-346) is wrapped to record every fixed-k MILP it issues
and HiGHS's answer. Nothing from the reference is copied into the repo; only
inputs and outputs (data) are written:

  tests/golden/fixtures.json         per profile folder x kv_bits x mip_gap:
                                     HALDAResult + per-k (status, w, n, obj, nodes,
                                     dual bound, LP-relaxation objective) + CLI stdout
  tests/golden/synthetic_M{M}.json   seeded fleets (device dicts) + per-k results
  tests/golden/lowered.npz           the exact MILP arrays (c, A_ub CSR, b_ub, A_eq,
                                     bounds, integrality) for a few (fleet, k)
  tests/golden/ties.json             fleets of repeated devices (exact ties): the
                                     reference's own "same device twice" shape
                                     (test/test_integration.py:88, loaded by its
                                     cli.solver.load_devices_and_model) for every
                                     profile folder x kv_bits x mip_gap, and the tied
                                     synthetic fleets of tests/ties.py (copies / two /
                                     half) under two models: HALDAResult + per-k

  tests/golden/boundary.json         fleets whose one capacity row is delta bytes short of a whole number of
                                     layers, every row kind x kv 4bit / fp16 x a delta grid around HiGHS's
                                     integrality tolerance: HALDAResult + per-k with presolve on, and with
                                     presolve off where that differs (layout: tests/boundary.py)

Run `python tests/golden/gen_golden.py ties` to (re)write ties.json alone, `... boundary` for boundary.json
(~1 min on 8 cores; prints the cases per row kind, the in-window count and the reference_failure share).

Solver: scipy 1.15.3 / HiGHS 1.8.0 (git 222cce7), the version present here.
"""

from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import time
import types
import typing
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
REF_SRC = Path("/root/reference/src")
REF_ROOT = Path("/root/reference")

FOLDERS = ["hermes_70b", "llama_3_70b/4bit", "llama_3_70b/online", "qwen3_32b/bf16"]
KV = ["4bit", "8bit", "fp16"]
GAPS = [1e-4, 1e-9]
SYNTH = {1: 24, 2: 24, 3: 24, 4: 24, 8: 24, 16: 24, 32: 12, 64: 16}
LOWERED = [(1, 0, 40), (2, 3, 2), (3, 1, 4), (4, 0, 1), (4, 2, 5), (8, 5, 2), (16, 1, 1), (16, 2, 4),
           (64, 0, 1), (64, 0, 2)]


def import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF_SRC))
    shim = types.ModuleType("distilp.common.types")
    shim.ModelPhase = typing.Literal["merged", "prefill", "decode"]
    shim.QuantizationLevel = typing.Literal["Q4_K", "Q5_K", "Q6_K", "Q8_0", "BF16", "F16", "F32"]
    sys.modules["distilp.common.types"] = shim
    import distilp.solver.halda_p_solver as hp  # noqa: E402
    import cli.solver as cli  # noqa: E402
    from distilp.common import DeviceProfile, ModelProfileSplit  # noqa: E402
    return hp, cli, DeviceProfile, ModelProfileSplit


class MilpSpy:
    """Wraps scipy.optimize.milp inside the reference module; records each call."""

    def __init__(self, hp, keep_arrays=False):
        self.hp = hp
        self.real = hp.milp
        self.calls = []
        self.keep_arrays = keep_arrays

    def __call__(self, c, integrality, bounds, constraints, options):
        res = self.real(c=c, integrality=integrality, bounds=bounds, constraints=constraints, options=options)
        lp = self.real(c=c, integrality=np.zeros_like(integrality), bounds=bounds, constraints=constraints)
        M = (len(c) - 1) // 7
        rec = {
            "k": int(round(c[-1])) + 1,
            "status": int(res.status),
            "success": bool(res.success),
            "lp_status": int(lp.status),
            "lp_obj": float(lp.fun) if lp.success else None,
        }
        if res.success:
            x = np.asarray(res.x)
            rec.update(
                w=[int(round(v)) for v in x[:M]], n=[int(round(v)) for v in x[M:2 * M]],
                x=[float(v) for v in x], fun=float(res.fun), nodes=int(getattr(res, "mip_node_count", -1)),
                dual_bound=float(getattr(res, "mip_dual_bound", np.nan)), gap=float(getattr(res, "mip_gap", np.nan)),
            )
        if self.keep_arrays:
            rec["arrays"] = (np.array(c), np.array(integrality), bounds, constraints)
        self.calls.append(rec)
        return res

    def fixed_k(self, *args, **kwargs):
        """Wraps solve_fixed_k_milp to record the per-k obj_value (halda_p_solver.py:356-366)."""
        r = self.real_fixed_k(*args, **kwargs)
        self.calls[-1]["obj_value"] = float(r.obj_value)
        return r

    def __enter__(self):
        self.real_fixed_k = self.hp.solve_fixed_k_milp
        self.hp.milp = self
        self.hp.solve_fixed_k_milp = self.fixed_k
        return self

    def __exit__(self, *exc):
        self.hp.milp = self.real
        self.hp.solve_fixed_k_milp = self.real_fixed_k


def run_solve(hp, devs, model, kv, gap, keep_arrays=False):
    with MilpSpy(hp, keep_arrays) as spy:
        buf = io.StringIO()
        err = None
        with contextlib.redirect_stdout(buf):
            try:
                r = hp.halda_solve(devs, model, mip_gap=gap, plot=False, kv_bits=kv)
                result = {"w": r.w, "n": r.n, "k": r.k, "obj_value": r.obj_value, "sets": r.sets}
            except Exception as e:  # noqa: BLE001
                result, err = None, f"{type(e).__name__}: {e}"
    return result, err, spy.calls, buf.getvalue()


def cli_stdout(cli, argv):
    buf = io.StringIO()
    old = sys.argv
    sys.argv = ["solver"] + argv
    try:
        with contextlib.redirect_stdout(buf):
            code = cli.main()
    finally:
        sys.argv = old
    return code, buf.getvalue()


def strip_arrays(calls):
    return [{k: v for k, v in c.items() if k != "arrays"} for c in calls]


def main():
    hp, cli, DeviceProfile, ModelProfileSplit = import_reference()
    sys.path.append(str(REPO))
    from distilp_amd.synth import load_model_dict, synth_fleet  # our generator (data only)

    os.chdir(REF_ROOT)  # the reference CLI resolves "test/profiles/<name>" from cwd
    t0 = time.time()

    # ---- 1. profile-folder fixtures
    fixtures = {}
    for folder in FOLDERS:
        devs, model = cli.load_from_profile_folder(f"test/profiles/{folder}")
        for kv in KV:
            for gap in GAPS:
                res, err, calls, out = run_solve(hp, devs, model, kv, gap)
                fixtures[f"{folder}|{kv}|{gap:g}"] = {
                    "folder": folder, "kv_bits": kv, "mip_gap": gap, "result": res, "error": err,
                    "per_k": strip_arrays(calls), "stdout": out,
                }
    cli_cases = {}
    for name, argv in {
        "hermes_default": ["--profile", "hermes_70b", "--no-plot"],
        "online_default": ["--profile", "llama_3_70b/online", "--no-plot"],
        "online_quiet": ["--profile", "llama_3_70b/online", "--no-plot", "--quiet"],
        "qwen_verbose": ["--profile", "qwen3_32b/bf16", "--no-plot", "--verbose"],
        "online_gap": ["--profile", "llama_3_70b/online", "--no-plot", "--mip-gap", "1e-9"],
    }.items():
        code, out = cli_stdout(cli, argv)
        cli_cases[name] = {"argv": argv, "code": code, "stdout": out}
    (HERE / "fixtures.json").write_text(json.dumps({"fixtures": fixtures, "cli": cli_cases}, indent=1))
    print(f"fixtures done {time.time() - t0:.1f}s", file=sys.stderr)

    # ---- 2. synthetic fleets
    model_dict = load_model_dict()
    model = ModelProfileSplit.model_validate(model_dict).to_model_profile()
    lowered = {}
    for M, count in SYNTH.items():
        fleets = []
        for seed in range(count):
            devd = synth_fleet(seed, M)
            devs = [DeviceProfile.model_validate(d) for d in devd]
            want_arrays = {(M, seed, k) for (m_, s_, k) in LOWERED if m_ == M and s_ == seed for _ in [0]}
            res, err, calls, _ = run_solve(hp, devs, model, "4bit", 1e-4, keep_arrays=bool(want_arrays))
            for rec in calls:
                if (M, seed, rec["k"]) in want_arrays:
                    c, integ, bounds, cons = rec["arrays"]
                    key = f"M{M}_s{seed}_k{rec['k']}"
                    A_ub = np.asarray(cons[0].A)
                    nz = np.nonzero(A_ub)
                    lowered[key + "_c"] = c
                    lowered[key + "_integrality"] = integ.astype(np.uint8)
                    lowered[key + "_lb"] = np.asarray(bounds.lb, dtype=float)
                    lowered[key + "_ub"] = np.asarray(bounds.ub, dtype=float)
                    lowered[key + "_Aub_shape"] = np.array(A_ub.shape)
                    lowered[key + "_Aub_row"] = nz[0].astype(np.int32)
                    lowered[key + "_Aub_col"] = nz[1].astype(np.int32)
                    lowered[key + "_Aub_val"] = A_ub[nz]
                    lowered[key + "_bub"] = np.asarray(cons[0].ub, dtype=float)
                    lowered[key + "_Aeq"] = np.asarray(cons[1].A, dtype=float)
                    lowered[key + "_beq"] = np.asarray(cons[1].ub, dtype=float)
            fleets.append({"seed": seed, "devices": devd, "result": res, "error": err,
                           "per_k": strip_arrays(calls)})
        (HERE / f"synthetic_M{M}.json").write_text(json.dumps(
            {"M": M, "model": "llama_3_70b/online", "kv_bits": "4bit", "mip_gap": 1e-4, "fleets": fleets}))
        print(f"M={M} done {time.time() - t0:.1f}s", file=sys.stderr)
    np.savez_compressed(HERE / "lowered.npz", **lowered)


TIE_SEED0, TIE_N_EACH = 21000, 20  # tests/ties.py tied_fleets(20): 60 fleets
TIE_MODELS = {"llama_3_70b/online": None, "qwen3_32b/bf16": "test/profiles/qwen3_32b/bf16/model_profile.json"}


def tied_fleet_dicts(synth_fleet, tpl):
    """[(kind, seed, device dicts)] built exactly as tests/ties.py tied_fleets() builds its fleets."""
    import copy

    out = []
    for s in range(TIE_N_EACH):
        src = synth_fleet(TIE_SEED0 + s, 16, tpl)
        one = src[s % 2]
        out.append(("copies", s, [copy.deepcopy(one) for _ in range(16)]))
        out.append(("two", s, [copy.deepcopy(src[1]) for _ in range(8)] + [copy.deepcopy(src[2 + s % 14]) for _ in range(8)]))
        out.append(("half", s, copy.deepcopy(src[:8] + src[:8])))
    return out


def gen_ties():
    hp, cli, DeviceProfile, ModelProfileSplit = import_reference()
    sys.path.append(str(REPO))
    from distilp_amd.synth import load_model_dict, load_templates, synth_fleet  # our generator (data only)

    os.chdir(REF_ROOT)
    t0 = time.time()
    twice = {}
    for folder in FOLDERS:
        base = Path("test/profiles") / folder
        dev = sorted(p for p in base.glob("*.json") if p.name != "model_profile.json")[0]
        devs, model = cli.load_devices_and_model([str(dev), str(dev)], str(base / "model_profile.json"))
        for kv in KV:
            for gap in GAPS:
                res, err, calls, _ = run_solve(hp, devs, model, kv, gap)
                twice[f"{folder}|{kv}|{gap:g}"] = {"folder": folder, "device_file": dev.name, "kv_bits": kv,
                                                   "mip_gap": gap, "result": res, "error": err,
                                                   "per_k": strip_arrays(calls)}
    print(f"twice done {time.time() - t0:.1f}s", file=sys.stderr)
    tpl = load_templates()
    fleets = tied_fleet_dicts(synth_fleet, tpl)
    tied = {}
    for mname, mfile in TIE_MODELS.items():
        if mfile is None:
            model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
        else:
            model = cli.load_model_profile(mfile)
        rows = []
        for kind, seed, dicts in fleets:
            devs = [DeviceProfile.model_validate(d) for d in dicts]
            res, err, calls, _ = run_solve(hp, devs, model, "4bit", 1e-4)
            rows.append({"kind": kind, "seed": seed, "result": res, "error": err, "per_k": strip_arrays(calls)})
        tied[mname] = {"model": mname, "kv_bits": "4bit", "mip_gap": 1e-4, "fleets": rows}
        print(f"tied {mname} done {time.time() - t0:.1f}s", file=sys.stderr)
    (HERE / "ties.json").write_text(json.dumps({"twice": twice, "tied": tied, "seed0": TIE_SEED0,
                                                "n_each": TIE_N_EACH}))


# ---------------------------------------------------------------- boundary goldens
# Capacity rows a few bytes short of a whole number of layers: rhs = j b' - delta. In the reference
# every slack is an integer column, so HiGHS takes a slack of delta / b' <= ~1e-6 (its integrality
# tolerance) as the integer 0; the grid below brackets that window for every kind of capacity row.
B_KV = ["4bit", "fp16"]
B_FIXED = [-10, -1, 0, 1, 10, 100, 300, 1000, 3000, 10000]
B_REL = [0.5, 0.9, 1.1, 2.0, 20.0]  # x T, T = 1e-6 b'
B_FAIL_CAP = 0.10
# base fleets and the (device, row kind) boundaries tried on each (kept where binding, <= 2 j each): the four
# profile folders, and synthetic fleets (M, seed, mods, targets); a mod sets fields of one device before the
# boundary edit (os_type "linux" on a Metal device: a Metal VRAM row without an M2 row)
B_FOLDERS = {"hermes_70b": [(0, "M2")], "llama_3_70b/4bit": [(0, "M2")], "llama_3_70b/online": [(0, "M2")],
             "qwen3_32b/bf16": [(0, "metal_vram")]}
B_SYNTH = [(2, 0, [], [(1, "M3")]), (2, 0, [{"dev": 1, "set": {"os_type": "mac_no_metal"}}], [(1, "M1")]),
           (2, 2, [], [(1, "cuda_vram")]), (2, 5, [], [(0, "M2")]),
           (4, 3, [], [(3, "M3_android")]),
           (4, 6, [{"dev": 0, "set": {"os_type": "linux"}}, {"dev": 3, "set": {"os_type": "linux"}}],
            [(0, "metal_vram"), (3, "metal_vram")]),
           (16, 1, [], [(3, "cuda_vram"), (6, "metal_vram")]), (16, 2, [], [(1, "cuda_vram"), (2, "metal_vram")])]


def _b_rows(mo, devs, model, kvf):
    """[(device, kind, row index)] of the capacity rows of oracle.milp_oracle.lower_dense, by pattern."""
    p = mo.lower_dense(devs, model, 1, kvf)
    M = p["M"]
    out = []
    for r in range(p["A_ub"].shape[0]):
        row = p["A_ub"][r]
        if row[7 * M] != 0.0:
            continue
        blk = [b for b in range(2, 6) if np.any(row[b * M:(b + 1) * M] != 0.0)]
        if not blk:
            continue  # link row
        i = int(np.nonzero(row[blk[0] * M:(blk[0] + 1) * M])[0][0])
        d = devs[i]
        if blk[0] == 2:
            kind = "M1"
        elif blk[0] == 3:
            kind = "M2"
        elif blk[0] == 4:
            kind = "M3_android" if d.os_type == "android" else "M3"
        else:
            prior = [k for (j, k, _) in out if j == i and k.endswith("vram")]
            kind = "cuda_vram" if (d.has_cuda and d.d_avail_cuda is not None and not prior) else "metal_vram"
        out.append((i, kind, r))
    return p, out


def _b_field(kind):
    return {"M1": "d_avail_ram", "M2": "d_avail_metal", "M3": "d_avail_ram", "M3_android": "d_swap_avail",
            "cuda_vram": "d_avail_cuda", "metal_vram": "d_avail_metal"}[kind]


def _b_apply(dicts, i, edits):
    import copy

    out = copy.deepcopy(dicts)
    out[i].update(edits)
    return out


def _b_case_edits(mo, DeviceProfile, dicts, model, kvf, i, kind, j, delta, how):
    """Edits of device i that put its `kind` row at rhs = j b' - delta (the integer field rounded to
    nearest, or so that the achieved delta is <= / >= the target: how = "le" / "ge"); plus the achieved
    rhs and delta as lower_dense gives them, b' and {row kind: achieved delta} of every row the field feeds."""
    import math

    field = _b_field(kind)
    base = {}
    if kind == "M3_android":
        # swap term active: RAM half a GB under the boundary, the rest from swap (min(can_swap, swap_avail))
        bp = mo._bprime(model, kvf)
        base = {"d_avail_ram": int(j * bp - 500_000_000), "d_bytes_can_swap": 1 << 40}
    d0 = _b_apply(dicts, i, {**base, field: 1_000_000_000 if kind == "M3_android" else dicts[i][field]})
    devs = [DeviceProfile.model_validate(d) for d in d0]
    p, rows = _b_rows(mo, devs, model, kvf)
    r = next(r for (ii, k, r) in rows if ii == i and k == kind)
    bp = float(p["A_ub"][r][i] if kind not in ("cuda_vram", "metal_vram") else p["A_ub"][r][p["M"] + i])
    off = float(d0[i][field]) - float(p["b_ub"][r])  # field - rhs
    want = j * bp - delta + off
    val = {"le": math.ceil, "ge": math.floor, "round": round}[how](want)
    edits = {**base, field: int(val)}
    d1 = _b_apply(dicts, i, edits)
    devs = [DeviceProfile.model_validate(d) for d in d1]
    p, rows = _b_rows(mo, devs, model, kvf)
    rhs = float(p["b_ub"][r])
    # every row of the device that the edited field feeds, with its own achieved delta
    moved = {k: float(j * bp - float(p["b_ub"][rr])) for (ii, k, rr) in rows if ii == i and _b_field(k) == field}
    return edits, d1, rhs, float(j * bp - rhs), bp, moved


class BoundarySpy(MilpSpy):
    """MilpSpy without the LP relaxation; records obj_value_rint and, on request, a presolve-off re-solve."""

    def __init__(self, hp, nopre):
        super().__init__(hp)
        self.nopre = nopre

    @staticmethod
    def _rec(res, c, cons):
        M = (len(c) - 1) // 7
        rec = {"status": int(res.status), "success": bool(res.success)}
        if res.success:
            x = np.asarray(res.x, dtype=float)
            rec["w"] = [int(round(v)) for v in x[:M]]
            rec["n"] = [int(round(v)) for v in x[M:2 * M]]
            rec["_lin"] = float(np.dot(c, x))
            # integer columns rounded; the continuous z, C re-minimised for them (closed form: the
            # stall columns occur only in their device's two cycle rows)
            xi = np.rint(x[:6 * M])
            A, ub = np.asarray(cons[0].A), np.asarray(cons[0].ub, dtype=float)
            iC = 7 * M
            C = 0.0
            for i in range(M):
                P = Q = None
                for r in np.nonzero(A[:, 6 * M + i])[0]:
                    act = float(np.dot(A[r, :6 * M], xi)) - ub[r]
                    if A[r, 6 * M + i] > 0:
                        P = act
                    else:
                        Q = act
                C = max(C, P, 0.5 * (P + Q))
            rec["_lin_rint"] = rec["lin_rint"] = float(np.dot(c[:6 * M], xi)) + float(c[iC]) * C
        return rec

    def __call__(self, c, integrality, bounds, constraints, options):
        res = self.real(c=c, integrality=integrality, bounds=bounds, constraints=constraints, options=options)
        rec = self._rec(res, c, constraints)
        rec["k"] = int(round(c[-1])) + 1
        if self.nopre:
            res2 = self.real(c=c, integrality=integrality, bounds=bounds, constraints=constraints,
                             options={**options, "presolve": False})
            rec["_nopre"] = self._rec(res2, c, constraints)
        self.calls.append(rec)
        return res

    def fixed_k(self, *args, **kwargs):
        r = self.real_fixed_k(*args, **kwargs)
        rec = self.calls[-1]
        rec["obj_value"] = float(r.obj_value)
        const = float(r.obj_value) - rec["_lin"]
        rec["obj_value_rint"] = rec["_lin_rint"] + const
        rec["_const"] = const
        return r


def _b_clean(rec):
    return {k: v for k, v in rec.items() if not k.startswith("_")}


def _b_solve(hp, devs, model, kv, nopre, const=None):
    """(result, per_k, per_k presolve-off or None) of the reference's halda_solve. The presolve-off
    records take the objective constant (the same for every k) from a presolve-on solve of the call,
    or `const` when every one of those failed."""
    with BoundarySpy(hp, nopre) as spy:
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                r = hp.halda_solve(devs, model, mip_gap=1e-4, plot=False, kv_bits=kv)
                result = {"w": r.w, "n": r.n, "k": r.k, "obj_value": r.obj_value, "_sets": r.sets}
            except Exception:  # noqa: BLE001
                result = None
    per_k = [_b_clean(c) for c in spy.calls]
    off = None
    if nopre:
        off = []
        const = next((c["_const"] for c in spy.calls if "_const" in c), const)
        for c in spy.calls:
            q = c["_nopre"]
            if q["success"]:
                q["obj_value"] = q["_lin"] + const
                q["obj_value_rint"] = q["_lin_rint"] + const
            q = _b_clean(q)
            q["k"] = c["k"]
            off.append(q)
    return result, per_k, off


def _b_best(per_k):
    """The reference's argmin over k (ascending k, strict "<" on obj_value) of a per-k list."""
    best = None
    for r in per_k:
        if r["success"] and (best is None or r["obj_value"] < best["obj_value"]):
            best = r
    return None if best is None else {"w": best["w"], "n": best["n"], "k": best["k"], "obj_value": best["obj_value"]}


def _b_key(res):
    return None if res is None else (res["k"], res["w"], res["n"])


_B = {}


def _b_obj(r):
    return r["obj_value_rint"] if "obj_value_rint" in r else r["obj_value"]


def _b_same(a, b):
    """Two per-k lists agree: status, (w, n), and the objective at the rounded integer columns to 1e-9."""
    return all(u["success"] == v["success"] and (not u["success"] or (
        (u["w"], u["n"]) == (v["w"], v["n"]) and abs(_b_obj(u) - _b_obj(v)) <= 1e-9 * max(1.0, abs(_b_obj(v)))))
        for u, v in zip(a, b))


def _b_unit(unit):
    """One (base fleet, kv): of its targets keep the binding (device, row, j) groups, run the delta grid on each."""
    hp, cli, DeviceProfile, ModelProfileSplit, mo, OurDev = _B["env"]
    name, dicts, model, kv, targets = unit
    kvf = mo._kv_factor(kv)
    T = 1e-6 * mo._bprime(model, kvf)

    def ref_devs(dd):
        return [DeviceProfile.model_validate(d) for d in dd]

    base, _, _ = _b_solve(hp, ref_devs(dicts), model, kv, False)
    if base is None:
        return []
    groups = []
    for (i, kind) in targets:
        w, n = base["w"][i], base["n"][i]
        q = {"M1": w, "M2": w, "M3": w - n, "M3_android": w - n, "cuda_vram": n, "metal_vram": n}[kind]
        kept = []
        for j in (q, q - 1, q + 1, q - 2):
            if j < 1 or len(kept) >= 2:
                continue
            ans = []
            for delta in (-10, 10000):
                _, d1, _, _, _, _ = _b_case_edits(mo, OurDev, dicts, model, kvf, i, kind, j, delta, "round")
                r, _, _ = _b_solve(hp, ref_devs(d1), model, kv, False)
                ans.append(_b_key(r))
            if ans[0] is not None and ans[1] is not None and ans[0] != ans[1]:
                kept.append(j)
        groups += [(i, kind, j) for j in kept]
    out = []
    for (i, kind, j) in groups:
        grid = [(float(d), "round") for d in B_FIXED if not (0.9 * T < d < 1.1 * T)]
        grid += [(f * T, "le" if f < 1 else "ge") for f in B_REL]
        cases = []
        for delta, how in grid:
            edits, d1, rhs, got, bpf, moved = _b_case_edits(mo, OurDev, dicts, model, kvf, i, kind, j, delta, how)
            ours = [OurDev.model_validate(d) for d in d1]
            res, per_k, off = _b_solve(hp, ref_devs(d1), model, kv, True,
                                       const=float(sum(mo.lower_dense(ours, model, 1, kvf)["const"])))
            _, ex_k = mo.halda_solve_oracle(ours, model, mip_gap=1e-4, kv_bits=kv, solver="exact")
            same_off, off_eq_exact, on_eq_exact = _b_same(per_k, off), _b_same(off, ex_k), _b_same(per_k, ex_k)
            # reference_failure: HiGHS's presolve changes the answer on a row within 2 B of a whole number of
            # layers, and without presolve HiGHS agrees with the exact solver. reference_unstable: presolve
            # changes the answer anywhere else; `match` says which of the two HiGHS answers is the exact optimum
            # under the slack rule ("a_nopre" / "a"), or none (the exact solver's must then be no worse).
            cls = "ok" if same_off else ("reference_failure" if off_eq_exact and abs(got) <= 2.0
                                         else "reference_unstable")
            case = {"delta_target": delta, "edits": edits, "rhs": rhs, "delta": got, "class": cls, "result": res,
                    "per_k": per_k, "delta_rows": {k: v for k, v in moved.items() if k != kind},
                    "_exact_ok": on_eq_exact if cls == "ok" else True}
            if cls != "ok":
                case["nopre"], case["result_nopre"] = off, _b_best(off)
            if cls == "reference_unstable":
                case["match"] = "a_nopre" if off_eq_exact else ("a" if on_eq_exact else None)
                if case["match"] is None:  # the exact optimum against the better of the two HiGHS answers, per k
                    case["_gap"] = max((e["obj_value"] - min(_b_obj(r) for r in (u, v) if r["success"]))
                                       / abs(e["obj_value"]) for u, v, e in zip(per_k, off, ex_k)
                                       if u["success"] or v["success"])
            cases.append(case)
        anchors = [c for c in cases if c["delta_target"] in (-10.0, 10000.0)]
        if any(c["class"] != "ok" for c in anchors) or _b_key(anchors[0]["result"]) == _b_key(anchors[1]["result"]):
            continue  # the group's two reference answers must themselves be stable and differ
        out.append({"fleet": name, "kv_bits": kv, "device": i, "row": kind, "rows_moved": sorted(moved), "j": j,
                    "b_prime": bpf, "T": 1e-6 * bpf, "head": bool(dicts[i]["is_head"]), "cases": cases})
    return out


def gen_boundary(jobs=8):
    import multiprocessing as mp

    hp, cli, DeviceProfile, ModelProfileSplit = import_reference()
    sys.path.append(str(REPO))
    from distilp_amd.common import DeviceProfile as OurDev
    from distilp_amd.synth import load_model_dict, synth_fleet
    from oracle import milp_oracle as mo

    os.chdir(REF_ROOT)
    t0 = time.time()
    _B["env"] = (hp, cli, DeviceProfile, ModelProfileSplit, mo, OurDev)
    fleets = {}
    units = []
    for folder in FOLDERS:
        base = Path("test/profiles") / folder
        files = sorted(p for p in base.glob("*.json") if p.name != "model_profile.json")
        dicts = [json.loads(p.read_text()) for p in files]
        dicts[0]["is_head"] = True  # as load_from_profile_folder marks it
        model = cli.load_model_profile(str(base / "model_profile.json"))
        fleets[folder] = {"folder": folder}
        for kv in B_KV:
            units.append((folder, dicts, model, kv, B_FOLDERS[folder]))
    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    for M, seed, mods, targets in B_SYNTH:
        dicts = synth_fleet(seed, M)
        for m in mods:
            dicts[m["dev"]].update(m["set"])
        name = f"synth_M{M}_s{seed}" + ("_" + "_".join(f"{m['dev']}{m['set']['os_type']}" for m in mods) if mods else "")
        fleets[name] = {"M": M, "seed": seed, "mods": mods}
        for kv in B_KV:
            units.append((name, dicts, model, kv, targets))
    units.sort(key=lambda u: -len(u[1]))
    with mp.get_context("fork").Pool(jobs) as pool:
        parts = pool.map(_b_unit, units, chunksize=1)
    groups = [g for part in parts for g in part]
    groups.sort(key=lambda g: (list(fleets).index(g["fleet"]), g["kv_bits"], g["device"], g["row"], g["j"]))
    n = fails = unstable = window = window_ok = bad = 0
    kinds = {}
    for g in groups:
        for c in g["cases"]:
            n += 1
            kinds[g["row"]] = kinds.get(g["row"], 0) + 1
            fails += c["class"] == "reference_failure"
            unstable += c["class"] == "reference_unstable"
            inw = 1e-9 * g["b_prime"] < c["delta"] <= 0.9 * g["T"]
            window += inw
            window_ok += inw and c["class"] == "ok"
            if "_gap" in c:
                print(f"  unstable, neither HiGHS answer is the exact optimum: {g['fleet']} {g['kv_bits']} dev "
                      f"{g['device']} {g['row']} j {g['j']} delta {c['delta']:.3f}: exact - best HiGHS = "
                      f"{c.pop('_gap'):.3e} relative", file=sys.stderr)
            if not c.pop("_exact_ok"):
                bad += 1
                print(f"  exact oracle (eps {mo.SLACK_EPS:g}) differs: {g['fleet']} {g['kv_bits']} dev {g['device']} "
                      f"{g['row']} j {g['j']} delta {c['delta']:.3f}", file=sys.stderr)
    print(f"boundary: {n} cases in {len(groups)} groups, per row kind {kinds}; in window {window} ({window_ok} ok); "
          f"reference_failure {fails} ({100.0 * fails / max(n, 1):.1f} %); reference_unstable {unstable} "
          f"({100.0 * unstable / max(n, 1):.1f} %); ok cases the exact oracle (eps {mo.SLACK_EPS:g}) misses {bad}; "
          f"{time.time() - t0:.0f}s")
    assert fails <= B_FAIL_CAP * n, "reference_failure share above the cap: thin the delta in {-1, 0, 1} points"
    for g in groups:
        g["ks"] = [r["k"] for r in g["cases"][0]["per_k"]]
        g["sets"] = g["cases"][0]["result"]["_sets"]  # (the -10 B anchor: always solved)
        for c in g["cases"]:
            assert c["result"] is None or c["result"].pop("_sets") == g["sets"]
        assert all([r["k"] for r in c["per_k"]] == g["ks"] for c in g["cases"])
        g["answers"] = []
        g["cases"] = [_b_pack(g, c) for c in g["cases"]]
    (HERE / "boundary.json").write_text(json.dumps(
        {"mip_gap": 1e-4, "fleets": fleets, "groups": groups}, separators=(",", ":")))


def _b_answer(g, per_k):
    """Index in g["answers"] of a per-k answer (parallel arrays over g["ks"]: HiGHS status, w, n and lin_rint,
    the reference's c.x at its rounded integer columns). The cases of a group share a few distinct answers."""
    a = {"status": [r["status"] for r in per_k], "w": [r.get("w") for r in per_k], "n": [r.get("n") for r in per_k],
         "lin_rint": [r.get("lin_rint") for r in per_k]}
    if a not in g["answers"]:
        g["answers"].append(a)
    return g["answers"].index(a)


def _b_pack(g, c):
    """A case as written: its per-k answers by index; `const`, the objective's constant (obj_value_rint =
    lin_rint + const); `excess`, {position: obj_value - obj_value_rint} where HiGHS's own objective carries
    the price of a fractional slack; of the results, k and obj_value (w, n: the answer's at that k)."""
    ok = [r for r in c["per_k"] + c.get("nopre", []) if r["success"]]
    out = {"delta_target": round(c["delta_target"], 3), "edits": c["edits"], "rhs": c["rhs"],
           "delta": round(c["delta"], 7)}
    if c["class"] != "ok":
        out["class"] = c["class"]  # (absent: "ok")
    out["const"] = ok[0]["obj_value_rint"] - ok[0]["lin_rint"] if ok else None
    out["a"] = _b_answer(g, c["per_k"])
    excess = {str(j): float(f"{r['obj_value'] - r['obj_value_rint']:.3e}") for j, r in enumerate(c["per_k"])
              if r["success"] and abs(r["obj_value"] - r["obj_value_rint"]) > 1e-12 * abs(r["obj_value_rint"])}
    if excess:
        out["excess"] = excess
    out["result"] = None if c["result"] is None else {"k": c["result"]["k"], "obj_value": c["result"]["obj_value"]}
    if c["delta_rows"]:
        out["delta_rows"] = {k: round(v, 7) for k, v in c["delta_rows"].items()}
    if c["class"] == "reference_unstable":
        out["match"] = c["match"]
    if "nopre" in c:
        out["a_nopre"] = _b_answer(g, c["nopre"])
    if "result_nopre" in c:
        r = c["result_nopre"]
        out["result_nopre"] = None if r is None else {"k": r["k"], "obj_value": r["obj_value"]}
    return out


if __name__ == "__main__":
    if sys.argv[1:] == ["ties"]:
        gen_ties()
    elif sys.argv[1:] == ["boundary"]:
        gen_boundary()
    else:
        main()
