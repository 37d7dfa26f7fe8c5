"""A/B of halda_solve_fleets_bounded: the fused route against the general route and the unbounded sweep, one build.

By HIP events around one call on resident device arrays (best_k, obj_value, w, n), the legs alternated over
ROUNDS rounds of REPS calls each (the median of every round, then the median and the spread of the rounds):
  (a) 4,096 fleets x 64 devices (C3's shape; a synthetic table tiled and re-profiled per fleet), the bounds the
      D = 2 box around the k = 1 optimum of a perturbed() copy: the unbounded sweep (the yardstick), the fused
      bounded launch (halda_sweep_bounds_kernel) and the general route (halda_set_bounds_path(1): lowering,
      halda_bound_cols_kernel, the CSR pipeline);
  (b) 4,096 fleets x 16 devices (C2's shape): the general route is the only one; against the unbounded sweep.
And end to end, wall clock, (c): halda_solve_bounded_batch of 128 fleets x 64 devices against a Python loop over
host-lowered fleets with their w column bounds patched, solved through halda_solve_batch's CSR entry.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/bounds_ab.py --out profiles/bounds_ab.json
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
N_FLEETS, N_BASE = 4096, 32


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import bounds as bd
    from distilp_amd.solver import halda_solve_bounded_batch
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.batch import assemble
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, FleetTable, HaldaBoundsC, HaldaFleetResultC,
                                           _fleets_struct, fleet_table, model_struct, solve_table)
    from distilp_amd.solver.lower import lower_fleet
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    ks = sorted(k for k in range(1, model.L) if model.L % k == 0)
    karr = np.asarray(ks, np.int32)
    stream = torch.cuda.Stream(dev)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS}
    fields = ("os_class", "flags") + F64_FIELDS + BYTE_FIELDS

    def big_table(M, seed):
        """N_FLEETS fleets of M devices: N_BASE synthetic fleets tiled, every fleet re-profiled on its own."""
        base = fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(seed + s, M)]
                            for s in range(N_BASE)], model)
        t = FleetTable(dev_off=np.arange(N_FLEETS + 1, dtype=np.int64) * M,
                       **{f: np.tile(getattr(base, f), N_FLEETS // N_BASE) for f in fields})
        return t.perturbed(np.random.default_rng(seed))

    for name, M in (("a_c3_4096x64", 64), ("b_c2_4096x16", 16)):
        table = big_table(M, 1000 + M)
        inc = solve_table(table.perturbed(np.random.default_rng(7)), model, [1], 0.5)
        lo = np.maximum(1, inc.w - 2).astype(np.int32)
        hi = (inc.w + 2).astype(np.int32)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nf, nd = table.n_fleets, table.n_devices
        i32, f64 = torch.int32, torch.float64
        o = [torch.empty(nf, dtype=i32, device=dev), torch.empty(nf, dtype=f64, device=dev),
             torch.empty(nd, dtype=i32, device=dev), torch.empty(nd, dtype=i32, device=dev)]
        bt = [torch.from_numpy(a).to(dev) for a in (lo, hi)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
        bc = HaldaBoundsC(*[t.data_ptr() for t in bt])
        m = model_struct(model, 0.5)

        def leg(kind):
            bd.set_bounds_path(ctx, 1 if kind == "general" else 0)
            ts = []
            for rep in range(WARM + REPS):
                for t in o:
                    t.fill_(-7)
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

        legs = ("sweep", "bounded", "general")
        rounds = {k: [] for k in legs}
        res, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in legs:
                ms_med, routes[kind], res[kind] = leg(kind)
                rounds[kind].append(ms_med * 1e3)
        bd.set_bounds_path(ctx, 0)
        med = {k: statistics.median(rounds[k]) for k in legs}
        out[name] = {"workload": f"{nf} fleets x {M} devices, {len(ks)} k, D = 2 boxes", "routes": routes,
                     "same_plans_bounded_general": all(np.array_equal(a, b) for a, b in
                                                       zip(res["bounded"][:1] + res["bounded"][2:],
                                                           res["general"][:1] + res["general"][2:])),
                     "max_rel_obj_bounded_general": float(np.max(np.abs(res["bounded"][1] - res["general"][1])
                                                                 / np.abs(res["general"][1]))),
                     "fleets_whose_plan_differs_from_the_sweep": int(
                         (res["bounded"][2].reshape(nf, M) != res["sweep"][2].reshape(nf, M)).any(axis=1).sum()),
                     "feasible": int((res["bounded"][0] > 0).sum()),
                     "bounded_over_sweep": med["bounded"] / med["sweep"],
                     "general_over_bounded": med["general"] / med["bounded"],
                     **{f"{k}_event_us": med[k] for k in legs}, **{f"{k}_rounds_us": rounds[k] for k in legs}}

    # (c) end to end
    fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(2000 + s, 64)] for s in range(128)]
    old = solve_table(fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(3000 + s, 64)]
                                   for s in range(128)], model), model, [1], 0.5)
    boxes = [bd.move_bounds(old.w[64 * f:64 * f + 64].tolist(), 2) for f in range(128)]

    def timed(fn):
        for _ in range(2):
            res = fn()
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, res

    def by_hand():
        plans = []
        for devs, (blo, bhi) in zip(fleets, boxes):
            batch, refs = assemble([lower_fleet(devs, model, kv_factor=0.5)], [[1]], mip_gap=0.0)
            batch.col_lb[:64] = blo
            batch.col_ub[:64] = np.minimum(bhi, refs[0].W)
            got = ctx.solve(batch)
            plans.append(np.rint(got.x[:64]).astype(int).tolist() if got.status[0] == 0 else None)
        return plans

    a_ms, a_all, a_res = timed(lambda: halda_solve_bounded_batch(fleets, model, boxes, [1], kv_bits="4bit"))
    b_ms, b_all, b_res = timed(by_hand)
    out["c_end_to_end_128x64"] = {
        "halda_solve_bounded_batch_ms": a_ms, "halda_solve_bounded_batch_all_ms": a_all,
        "host_lowered_patched_loop_ms": b_ms, "host_lowered_patched_loop_all_ms": b_all,
        "same_plans": [None if x is None else x.w for x in a_res] == b_res}
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
