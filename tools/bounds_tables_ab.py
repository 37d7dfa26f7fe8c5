"""A/B of halda_solve_fleets_bounded's table route (bounds path 3, halda_sweep_bounds_tables_kernel) against the
general route and the unbounded sweep, one build.

By HIP events around one call on resident device arrays (best_k, obj_value, w, n), warm, the legs alternated
over ROUNDS rounds of REPS calls each (the median of every round, then the median and the spread of the rounds),
on the 80-layer model with D = 2 boxes around the optimum of a perturbed() copy of the table over the same k:
  4,096 fleets x 16 devices, ks = [2];  4,096 x 16, ks = [1, 2, 4, 5];  4,096 x 8, ks = [2];  256 x 16, ks = [2].
Per shape: the unbounded sweep (the yardstick), the general route (halda_set_bounds_path(1): lowering,
halda_bound_cols_kernel, the CSR pipeline, the pick kernel) and the table route (path 3, one launch).
And end to end, wall clock: halda_solve_bounded_batch of 128 fleets x 16 devices at ks = [2], route="general"
against route="tables".
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/bounds_tables_ab.py --out profiles/bounds_tables_ab.json
"""

from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
WARM, REPS, ROUNDS = 3, 15, 5
N_BASE = 32
SHAPES = (("a_4096x16_k2", 4096, 16, [2]), ("b_4096x16_k1245", 4096, 16, [1, 2, 4, 5]),
          ("c_4096x8_k2", 4096, 8, [2]), ("d_256x16_k2", 256, 16, [2]))
LEGS = ("sweep", "general", "tables")


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import bounds as bd
    from distilp_amd.solver import halda_solve_bounded_batch
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, FleetTable, HaldaBoundsC, HaldaFleetResultC,
                                           _fleets_struct, fleet_table, model_struct, solve_table)
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

    for name, nf, M, ks in SHAPES:
        table = big_table(nf, M, 1000 + M)
        karr = np.asarray(ks, np.int32)
        inc = solve_table(table.perturbed(np.random.default_rng(7)), model, ks, 0.5)
        lo = np.maximum(1, inc.w - 2).astype(np.int32)
        hi = (inc.w + 2).astype(np.int32)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nd = table.n_devices
        i32, f64 = torch.int32, torch.float64
        o = [torch.empty(nf, dtype=i32, device=dev), torch.empty(nf, dtype=f64, device=dev),
             torch.empty(nd, dtype=i32, device=dev), torch.empty(nd, dtype=i32, device=dev)]
        bt = [torch.from_numpy(a).to(dev) for a in (lo, hi)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
        bc = HaldaBoundsC(*[t.data_ptr() for t in bt])
        m = model_struct(model, 0.5)

        def leg(kind):
            bd.set_bounds_path(ctx, {"general": 1, "tables": 3}.get(kind, 0))
            ts = []
            for rep in range(WARM + REPS):
                for t in o:
                    t.fill_(-7)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if kind == "sweep":
                    rc = lib.halda_solve_fleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, len(ks),
                                                ctypes.byref(r), ctypes.c_void_p(stream.cuda_stream))
                else:
                    rc = lib.halda_solve_fleets_bounded(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data,
                                                        len(ks), ctypes.byref(bc), ctypes.byref(r),
                                                        ctypes.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            route = bd.last_bounds_route(ctx) if kind != "sweep" else "sweep"
            return statistics.median(ts), route, [t.cpu().numpy().copy() for t in o]

        rounds = {k: [] for k in LEGS}
        res, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in LEGS:
                ms_med, routes[kind], res[kind] = leg(kind)
                rounds[kind].append(ms_med * 1e3)
        bd.set_bounds_path(ctx, 0)
        med = {k: statistics.median(rounds[k]) for k in LEGS}
        ok = res["general"][0] > 0
        out[name] = {"workload": f"{nf} fleets x {M} devices, ks = {ks}, D = 2 boxes", "routes": routes,
                     "same_plans_tables_general": all(np.array_equal(a, b) for a, b in
                                                      zip(res["tables"][:1] + res["tables"][2:],
                                                          res["general"][:1] + res["general"][2:])),
                     "max_rel_obj_tables_general": float(np.max(np.abs(res["tables"][1][ok] - res["general"][1][ok])
                                                                / np.abs(res["general"][1][ok]), initial=0.0)),
                     "fleets_whose_plan_differs_from_the_sweep": int(
                         (res["tables"][2].reshape(nf, M) != res["sweep"][2].reshape(nf, M)).any(axis=1).sum()),
                     "feasible": int((res["tables"][0] > 0).sum()),
                     "general_over_tables": med["general"] / med["tables"],
                     "tables_over_sweep": med["tables"] / med["sweep"],
                     "general_over_sweep": med["general"] / med["sweep"],
                     **{f"{k}_event_us": med[k] for k in LEGS}, **{f"{k}_rounds_us": rounds[k] for k in LEGS}}

    # end to end
    fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(2000 + s, 16)] for s in range(128)]
    old = solve_table(fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(3000 + s, 16)]
                                   for s in range(128)], model), model, [2], 0.5)
    boxes = [bd.move_bounds(old.w[16 * f:16 * f + 16].tolist(), 2) for f in range(128)]

    def timed(route):
        fn = lambda: halda_solve_bounded_batch(fleets, model, boxes, [2], kv_bits="4bit", route=route)
        for _ in range(2):
            res = fn()
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, res, bd.last_bounds_route(ctx)

    legs = {}
    for _ in range(2):  # alternate: the second round's figures are kept
        for route in ("general", "tables"):
            legs[route] = timed(route)
    key = lambda rs: [None if x is None else (x.k, x.w, x.n, x.obj_value) for x in rs]
    out["e_end_to_end_128x16_k2"] = {
        "routes": {k: v[3] for k, v in legs.items()},
        "general_ms": legs["general"][0], "general_all_ms": legs["general"][1],
        "tables_ms": legs["tables"][0], "tables_all_ms": legs["tables"][1],
        "general_over_tables": legs["general"][0] / legs["tables"][0],
        "same_results": key(legs["general"][2]) == key(legs["tables"][2])}
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
