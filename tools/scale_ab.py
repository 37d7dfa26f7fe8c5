"""Timing of halda_solve_change_subsets (scale-in: which devices to drop under a released-layer budget), beside the
two ways there were before.

Two shapes on the 80-layer model at k = 1, every fleet holding its own optimum, d <= 2 devices dropped, P = 4:
  64 fleets x 16 devices (137 candidates per fleet);   8 fleets x 64 devices (2,081 candidates per fleet).
Per shape
  by HIP events, warm, on resident device arrays, the legs alternated over ROUNDS rounds of REPS calls (the median
  of every round, then the median of the rounds): `scale`, one halda_solve_change_subsets call (it forms the
  candidates, runs the change kernel per d and picks on the device; its window includes the read-back of dev_off and
  w0 for the gate), against `lists`, halda_solve_change per d over the SAME lists already packed and resident (no
  pick: the per-candidate frontiers stay on the device);
  end to end, by the wall clock from Python objects to Python objects, REPS_E2E calls after one warm call:
  halda_scale_in_frontier_batch against halda_failover_frontiers with every tuple enumerated on the host (one call
  per fleet, then the arg-min per (d, p) in Python).
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out, writes it.

    python tools/scale_ab.py --out profiles/scale_ab.json
"""

from __future__ import annotations

import argparse
import ctypes
import itertools
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
WARM, REPS, ROUNDS, REPS_E2E = 2, 5, 3, 2
SHAPES = (("a_64x16", 64, 16), ("b_8x64", 8, 64))
K, D, P = 1, 2, 4


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import change as ch
    from distilp_amd.solver import scale as sc
    from distilp_amd.solver import subsets as ss
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaChangeC, HaldaChangeFrontierC, _fleets_struct,
                                           fleet_table, model_struct, solve_table)
    from distilp_amd.solver.subfleets import HaldaSubfleetsC, pack_items
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS, "reps_end_to_end": REPS_E2E, "k": K,
           "max_drop": D, "max_p": P}
    fields = ("os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    i32, f64 = torch.int32, torch.float64
    W = int(model.L) // K
    for name, nf, M in SHAPES:
        fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(1000 + M + s, M)] for s in range(nf)]
        table = fleet_table(fleets, model)
        inc = solve_table(table, model, [K], 0.5)
        assert (inc.best_k == K).all()
        w_all = inc.w.astype(np.int32)
        ws = [w_all[int(table.dev_off[f]):int(table.dev_off[f + 1])].tolist() for f in range(nf)]
        ns = [inc.n[int(table.dev_off[f]):int(table.dev_off[f + 1])].tolist() for f in range(nf)]
        tops = sc.check_scale_gate([M] * nf, [list(range(M))] * nf, ws, W, K, 0, D, P)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        m = model_struct(model, 0.5)
        tw0 = torch.from_numpy(w_all).to(dev)
        pts = nf * (D + 1) * (P + 1)
        go = [torch.empty(pts, dtype=i32, device=dev), torch.empty(pts, dtype=f64, device=dev),
              torch.empty(pts, dtype=torch.int64, device=dev), torch.empty(pts, dtype=i32, device=dev),
              torch.empty(pts, dtype=i32, device=dev), torch.empty(pts * 64, dtype=i32, device=dev),
              torch.empty(pts * 64, dtype=i32, device=dev)]
        sub = sc.HaldaChangeSubsetsC(tw0.data_ptr(), None, None, 0, D, P, None)
        grid = sc.HaldaChangeSubsetFrontierC(*[t.data_ptr() for t in go])
        # the same lists, packed on the host once and resident: one halda_solve_change per d
        per_d, n_lists = [], 0
        for d in range(D + 1):
            items = [(f, kept) for f in range(nf) for _, kept in ss.candidate_lists(M, list(range(M)), d)]
            parent, sub_off, sub_idx = pack_items(table.sizes(), items)
            w0 = np.concatenate([np.asarray([ws[f][i] for i in kept], np.int32) for f, kept in items])
            n, tot = len(items), int(sub_off[-1])
            n_lists += n
            keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                    for a in (parent.astype(np.int32), sub_off, sub_idx.astype(np.int32), w0)]
            fo = [torch.empty(n * (P + 1), dtype=i32, device=dev), torch.empty(n * (P + 1), dtype=f64, device=dev),
                  torch.empty(n * (P + 1), dtype=i32, device=dev), torch.empty(n * (P + 1), dtype=i32, device=dev),
                  torch.empty((P + 1) * tot, dtype=i32, device=dev), torch.empty((P + 1) * tot, dtype=i32, device=dev)]
            per_d.append((HaldaSubfleetsC(n, M - d, M - d, *[t.data_ptr() for t in keep[:3]]),
                          HaldaChangeC(keep[3].data_ptr(), None, None, P, tops[d]),
                          HaldaChangeFrontierC(tot, *[t.data_ptr() for t in fo]), keep, fo))

        def call(kind):
            if kind == "scale":
                rc = lib.halda_solve_change_subsets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), K, ctypes.byref(sub),
                                                    ctypes.byref(grid), sp)
                if rc != 0:
                    raise RuntimeError(f"scale failed ({rc}): {last_error(lib)}")
                return
            for itc, chc, frc, _, _ in per_d:
                rc = lib.halda_solve_change(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(itc), K,
                                            ctypes.byref(chc), ctypes.byref(frc), sp)
                if rc != 0:
                    raise RuntimeError(f"lists failed ({rc}): {last_error(lib)}")

        def leg(kind):
            ts = []
            for rep in range(WARM + REPS):
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(kind)
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            return statistics.median(ts)

        legs = ("scale", "lists")
        rounds = {kd: [] for kd in legs}
        for _ in range(ROUNDS):
            for kd in legs:
                rounds[kd].append(leg(kd) * 1e3)
        med = {kd: statistics.median(rounds[kd]) for kd in legs}
        # the grid equals the arg-min over the per-list frontiers
        st = go[0].cpu().numpy().reshape(nf, D + 1, P + 1)
        gobj = go[1].cpu().numpy().reshape(nf, D + 1, P + 1)
        same = True
        for d, (_, _, _, _, fo) in enumerate(per_d):
            lo = fo[1].cpu().numpy().reshape(nf, -1, P + 1)
            same = same and bool(np.array_equal(lo.min(axis=1), gobj[:, d]))

        incs = [(K, ws[f], ns[f]) for f in range(nf)]

        def e2e_scale():
            return sc.halda_scale_in_frontier_batch(fleets, model, incs, D, P, kv_bits="4bit")

        def e2e_lists():
            res = []
            for f in range(nf):
                lost = [c for d in range(1, D + 1) for c in itertools.combinations(range(M), d)]
                frs = ch.halda_failover_frontiers(fleets[f], model, incs[f], P, lost, "4bit")
                rows = [[None] * (P + 1) for _ in range(D + 1)]
                for g, fr in zip(lost, frs):
                    for p, pt in enumerate(fr):
                        cur = rows[len(g)][p]
                        if pt.plan is not None and (cur is None or pt.obj_value < cur[1].obj_value):
                            rows[len(g)][p] = (g, pt)
                res.append(rows)
            return res

        wall = {}
        got = {}
        for kd, fn in (("scale", e2e_scale), ("lists", e2e_lists)):
            fn()
            ts = []
            for _ in range(REPS_E2E):
                t0 = time.perf_counter()
                got[kd] = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            wall[kd] = ts
        agree = all(
            (got["lists"][f][d][p] is None) == (got["scale"][f][d][p].point.plan is None) and
            (got["lists"][f][d][p] is None or got["lists"][f][d][p][1].obj_value == got["scale"][f][d][p].point.obj_value)
            for f in range(nf) for d in range(1, D + 1) for p in range(P + 1))
        out[name] = {"workload": f"{nf} fleets x {M} devices, d <= {D}, P = {P}: {n_lists} candidate lists",
                     "max_deficit_per_d": tops, "cells_optimal": int((st == 0).sum()), "cells": int(st.size),
                     "grid_equals_min_over_lists": same, "end_to_end_cells_agree": bool(agree),
                     "scale_over_lists_events": med["scale"] / med["lists"],
                     **{f"{kd}_event_us": med[kd] for kd in legs}, **{f"{kd}_rounds_us": rounds[kd] for kd in legs},
                     "scale_end_to_end_ms": statistics.median(wall["scale"]),
                     "lists_end_to_end_ms": statistics.median(wall["lists"]),
                     "end_to_end_speedup": statistics.median(wall["lists"]) / statistics.median(wall["scale"]),
                     "scale_end_to_end_all_ms": wall["scale"], "lists_end_to_end_all_ms": wall["lists"]}
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=float, default=500.0, help="time limit of the GPU child process, seconds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child()
        return 0
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], capture_output=True, text=True,
                       timeout=args.timeout)
    sys.stderr.write(p.stderr)
    if p.returncode != 0:
        return p.returncode
    line = p.stdout.strip().splitlines()[-1]
    json.loads(line)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
