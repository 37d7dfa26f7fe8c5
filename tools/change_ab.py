"""Timing of halda_solve_change (halda_sweep_change_kernel), beside the free re-solve of the same items.

By HIP events around one call on resident device arrays, warm, the legs alternated over ROUNDS rounds of REPS
calls each (the median of every round, then the median and the spread of the rounds), on the 80-layer model.
The items are the leave-one-out lists of every fleet of the table (an N-1 contingency table), the survivors
holding the parent's own optimum at k:
  64 fleets x 16 devices (1,024 lists of 15) at k = 1 and k = 2, P = 4 and P = 8;
  64 fleets x 64 devices (4,096 lists of 63) at k = 1, P = 4.
Per shape the change launch (every point p = 0 .. P of every list in one launch) and, as the baseline,
halda_solve_subfleets of the same items at k_candidates = [k]: the free re-solve, the only answer there was
before, which gives ONE plan per list and may reshuffle every survivor.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/change_ab.py --out profiles/change_ab.json
"""

from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
WARM, REPS, ROUNDS = 2, 7, 3
SHAPES = (("a_64x16_k1_P4", 64, 16, 1, 4), ("b_64x16_k1_P8", 64, 16, 1, 8), ("c_64x16_k2_P4", 64, 16, 2, 4),
          ("d_64x16_k2_P8", 64, 16, 2, 8), ("e_64x64_k1_P4", 64, 64, 1, 4))
LEGS = ("change", "resolve")


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import change as ch
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaChangeC, HaldaChangeFrontierC,
                                           HaldaFleetResultC, _fleets_struct, fleet_table, model_struct, solve_table)
    from distilp_amd.solver.subfleets import HaldaSubfleetsC, last_subfleets_route, leave_one_out_items
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS}
    fields = ("os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    tables = {}
    for name, nf, M, k, P in SHAPES:
        if (nf, M) not in tables:
            tables[(nf, M)] = fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(1000 + M + s, M)]
                                           for s in range(nf)], model)
        table = tables[(nf, M)]
        inc = solve_table(table, model, [k], 0.5)
        assert (inc.best_k == k).all()
        parent, sub_off, sub_idx = leave_one_out_items(table.sizes())
        n, tot, P1 = len(parent), int(sub_off[-1]), P + 1
        g = np.repeat(table.dev_off[parent.astype(np.int64)], np.diff(sub_off)) + sub_idx
        w0 = inc.w[g].astype(np.int32)
        top = ch.check_w0(sub_off, w0, int(model.L) // k)
        ch.check_gate(M - 1, M - 1, P, top, k)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        i32, f64 = torch.int32, torch.float64
        m = model_struct(model, 0.5)
        karr = np.asarray([k], np.int32)
        it = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (parent.astype(np.int32), sub_off,
                                                                          sub_idx.astype(np.int32))]
        itc = HaldaSubfleetsC(n, M - 1, M - 1, *[t.data_ptr() for t in it])
        tw0 = torch.from_numpy(w0).to(dev)
        fo = [torch.empty(n * P1, dtype=i32, device=dev), torch.empty(n * P1, dtype=f64, device=dev),
              torch.empty(n * P1, dtype=i32, device=dev), torch.empty(n * P1, dtype=i32, device=dev),
              torch.empty(P1 * tot, dtype=i32, device=dev), torch.empty(P1 * tot, dtype=i32, device=dev)]
        chc = HaldaChangeC(tw0.data_ptr(), None, None, P, top)
        frc = HaldaChangeFrontierC(tot, *[t.data_ptr() for t in fo])
        o = [torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=f64, device=dev),
             torch.empty(tot, dtype=i32, device=dev), torch.empty(tot, dtype=i32, device=dev)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)

        def leg(kind):
            ts = []
            for rep in range(WARM + REPS):
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if kind == "change":
                    rc = lib.halda_solve_change(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(itc), k,
                                                ctypes.byref(chc), ctypes.byref(frc),
                                                ctypes.c_void_p(stream.cuda_stream))
                else:
                    rc = lib.halda_solve_subfleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(itc),
                                                   karr.ctypes.data, 1, ctypes.byref(r),
                                                   ctypes.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            return statistics.median(ts)

        rounds = {kd: [] for kd in LEGS}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in LEGS:
                rounds[kind].append(leg(kind) * 1e3)
        med = {kd: statistics.median(rounds[kd]) for kd in LEGS}
        st = fo[0].cpu().numpy().reshape(n, P1)
        obj = fo[1].cpu().numpy().reshape(n, P1)
        rel = fo[3].cpu().numpy().reshape(n, P1)
        free_obj = o[1].cpu().numpy()
        ok = (st[:, P] == 0) & (o[0].cpu().numpy() > 0)
        out[name] = {"workload": f"{nf} fleets x {M} devices: {n} leave-one-out lists of {M - 1}, k = {k}, P = {P} "
                                 f"({P1} points per list)",
                     "max_deficit": top, "lds_bytes_per_wave": ch.change_lds_bytes(M - 1, P, top, k),
                     "resolve_route": last_subfleets_route(ctx),
                     "points_optimal": int((st == 0).sum()), "points": int(st.size),
                     "frontier_non_increasing": bool((obj[:, 1:] <= obj[:, :-1]).all()),
                     "lists_that_release_at_P": int((rel[:, P] > 0).sum()),
                     # the free re-solve has no budget, so it is no worse than any point
                     "resolve_no_worse": bool((free_obj[ok] <= obj[ok, P] + 1e-9 * np.abs(obj[ok, P])).all()),
                     "lists_at_the_free_optimum_at_P": int((np.abs(free_obj[ok] - obj[ok, P])
                                                            <= 1e-9 * np.abs(obj[ok, P])).sum()),
                     "change_over_resolve": med["change"] / med["resolve"],
                     "change_us_per_list": med["change"] / n,
                     **{f"{kd}_event_us": med[kd] for kd in LEGS}, **{f"{kd}_rounds_us": rounds[kd] for kd in LEGS}}
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=float, default=400.0, help="time limit of the GPU child process, seconds")
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
