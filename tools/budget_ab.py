"""Timing of halda_solve_fleets_budget (halda_sweep_budget_kernel), beside the per-device box on the same shapes.

By HIP events around one call on resident device arrays, warm, the legs alternated over ROUNDS rounds of REPS
calls each (the median of every round, then the median and the spread of the rounds), on the 80-layer model
with the incumbent = the optimum of a perturbed() copy of the table at the same k:
  4,096 fleets x 16 devices at k = 1 and k = 2, P = 4 and P = 8;  4,096 x 64 at k = 1, P = 8.
Per shape the budget launch (every point p = 0 .. P in one launch) and, for scale, the per-device box of
halda_solve_fleets_bounded at D = P layers per device around the same incumbent (its automatic route: the table
launch, bounds path 3, where the fused register launch does not apply), which answers ONE box, not a frontier.
The parent build's own figures for the box are in profiles/bounds_tables_ab.json (table route) and
profiles/bounds_ab.json (fused route); this tool re-measures the box on this box so the two columns are from
one machine.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/budget_ab.py --out profiles/budget_ab.json
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
N_BASE = 32
SHAPES = (("a_4096x16_k1_P4", 4096, 16, 1, 4), ("b_4096x16_k1_P8", 4096, 16, 1, 8),
          ("c_4096x16_k2_P4", 4096, 16, 2, 4), ("d_4096x16_k2_P8", 4096, 16, 2, 8),
          ("e_4096x64_k1_P8", 4096, 64, 1, 8))
LEGS = ("budget", "box")


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import bounds as bd
    from distilp_amd.solver import budget as bg
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, FleetTable, HaldaBoundsC, HaldaBudgetC,
                                           HaldaFleetResultC, HaldaFrontierC, _fleets_struct, fleet_table,
                                           model_struct, solve_table)
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS}
    fields = ("os_class", "flags") + F64_FIELDS + BYTE_FIELDS

    def big_table(nf, M, seed):
        """nf fleets of M devices: N_BASE synthetic fleets tiled, every fleet re-profiled on its own."""
        base = fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(seed + s, M)]
                            for s in range(N_BASE)], model)
        t = FleetTable(dev_off=np.arange(nf + 1, dtype=np.int64) * M,
                       **{f: np.tile(getattr(base, f), nf // N_BASE) for f in fields})
        return t.perturbed(np.random.default_rng(seed))

    tables = {}
    for name, nf, M, k, P in SHAPES:
        if (nf, M) not in tables:
            tables[(nf, M)] = big_table(nf, M, 1000 + M)
        table = tables[(nf, M)]
        inc = solve_table(table.perturbed(np.random.default_rng(7)), model, [k], 0.5)
        w0 = inc.w.astype(np.int32)
        assert (inc.best_k == k).all()
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nd, P1 = table.n_devices, P + 1
        i32, f64 = torch.int32, torch.float64
        m = model_struct(model, 0.5)
        karr = np.asarray([k], np.int32)
        # the budget call
        tw0 = torch.from_numpy(w0).to(dev)
        fo = [torch.empty(nf * P1, dtype=i32, device=dev), torch.empty(nf * P1, dtype=f64, device=dev),
              torch.empty(nf * P1, dtype=i32, device=dev), torch.empty(P1 * nd, dtype=i32, device=dev),
              torch.empty(P1 * nd, dtype=i32, device=dev)]
        bgc = HaldaBudgetC(tw0.data_ptr(), None, None, P)
        frc = HaldaFrontierC(nd, *[t.data_ptr() for t in fo])
        # the per-device box D = P around the same incumbent
        bt = [torch.from_numpy(np.maximum(1, w0 - P).astype(np.int32)).to(dev), torch.from_numpy(w0 + P).to(dev)]
        o = [torch.empty(nf, dtype=i32, device=dev), torch.empty(nf, dtype=f64, device=dev),
             torch.empty(nd, dtype=i32, device=dev), torch.empty(nd, dtype=i32, device=dev)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
        bc = HaldaBoundsC(*[t.data_ptr() for t in bt])

        def leg(kind):
            ts = []
            for rep in range(WARM + REPS):
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if kind == "budget":
                    rc = lib.halda_solve_fleets_budget(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), k, ctypes.byref(bgc),
                                                       ctypes.byref(frc), ctypes.c_void_p(stream.cuda_stream))
                else:
                    rc = lib.halda_solve_fleets_bounded(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, 1,
                                                        ctypes.byref(bc), ctypes.byref(r),
                                                        ctypes.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            return statistics.median(ts)

        bd.set_bounds_path(ctx, 3)
        rounds = {kd: [] for kd in LEGS}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in LEGS:
                rounds[kind].append(leg(kind) * 1e3)
        route = bd.last_bounds_route(ctx)
        bd.set_bounds_path(ctx, 0)
        med = {kd: statistics.median(rounds[kd]) for kd in LEGS}
        st = fo[0].cpu().numpy().reshape(nf, P1)
        obj = fo[1].cpu().numpy().reshape(nf, P1)
        mv = fo[2].cpu().numpy().reshape(nf, P1)
        box_obj = o[1].cpu().numpy()
        ok = (st[:, P] == 0) & (o[0].cpu().numpy() > 0)
        out[name] = {"workload": f"{nf} fleets x {M} devices, k = {k}, P = {P} ({P1} points per fleet)",
                     "lds_bytes_per_wave": bg.budget_lds_bytes(M, P, k), "box_route": route,
                     "points_optimal": int((st == 0).sum()), "points": int(st.size),
                     "frontier_non_increasing": bool((np.diff(obj, axis=1) <= 0).all()),
                     "median_moved_layers_at_P": float(np.median(mv[:, P])),
                     "median_gain_point0_to_P": float(np.median(obj[:, 0] - obj[:, P])),
                     # the box D = P holds every plan of budget P, so its optimum is no worse
                     "box_no_worse_than_budget": bool((box_obj[ok] <= obj[ok, P] + 1e-9 * np.abs(obj[ok, P])).all()),
                     "budget_over_box": med["budget"] / med["box"],
                     "budget_us_per_fleet": med["budget"] / nf,
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
