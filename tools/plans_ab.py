"""A/B of halda_solve_fleets_plans: the fused route against the two-launch route and the bare sweep, on one build.

By HIP events around one call on resident device arrays (the sweep's best_k, obj_value, w, n and the
evaluation's status, obj_value, cycle, bottleneck, reason), the legs alternated over ROUNDS rounds of REPS calls
each (the median of every round, then the median and the spread of the rounds):
  (a) 4,096 fleets x 64 devices (C3's shape; a synthetic table tiled and re-profiled per fleet), incumbents =
      the optimum of a perturbed() copy: the fused route (halda_set_plans_path(2), halda_sweep_plans_kernel),
      the two-launch route (halda_set_plans_path(1): halda_eval_plans_kernel, then the sweep), and a bare
      halda_solve_fleets on the same table -- what the evaluation costs on top;
  (b) 4,096 fleets x 16 devices (C2's shape): the two-launch route is the only one; against the bare sweep.
And end to end, wall clock, (c): halda_replace_or_keep_batch against halda_solve_batch plus a Python loop of
evaluate_plan_np, on 128 fleets x 64 devices.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/plans_ab.py --out profiles/plans_ab.json
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
    from distilp_amd.solver import halda_replace_or_keep_batch, halda_solve_batch
    from distilp_amd.solver import plans as pl
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, FleetTable, HaldaFleetResultC, HaldaPlanResultC,
                                           HaldaPlansC, _fleets_struct, fleet_table, model_struct,
                                           solve_table)
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
        inc = solve_table(table.perturbed(np.random.default_rng(7)), model, ks, 0.5)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nf, nd = table.n_fleets, table.n_devices
        i32, f64 = torch.int32, torch.float64
        o = [torch.empty(nf, dtype=i32, device=dev), torch.empty(nf, dtype=f64, device=dev),
             torch.empty(nd, dtype=i32, device=dev), torch.empty(nd, dtype=i32, device=dev)]
        e = [torch.empty(nf, dtype=i32, device=dev), torch.empty(nf, dtype=f64, device=dev),
             torch.empty(nf, dtype=f64, device=dev), torch.empty(nf, dtype=i32, device=dev),
             torch.empty(nf, dtype=i32, device=dev)]
        plan = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev) for a in (inc.best_k, inc.w, inc.n)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
        er = HaldaPlanResultC(*[t.data_ptr() for t in e], None, None, None)
        pc = HaldaPlansC(*[t.data_ptr() for t in plan])
        m = model_struct(model, 0.5)

        def leg(kind):
            pl.set_plans_path(ctx, 1 if kind == "two_launch" else 2)
            ts = []
            for rep in range(WARM + REPS):
                for t in o + e:
                    t.fill_(-7)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if kind == "sweep":
                    rc = lib.halda_solve_fleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, len(ks),
                                                ctypes.byref(r), ctypes.c_void_p(stream.cuda_stream))
                else:
                    rc = lib.halda_solve_fleets_plans(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data,
                                                      len(ks), ctypes.byref(pc), ctypes.byref(er), ctypes.byref(r),
                                                      ctypes.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            route = pl.last_plans_route(ctx) if kind != "sweep" else "sweep"
            keep = o if kind == "sweep" else o + e
            return statistics.median(ts), route, [t.cpu().numpy().tobytes() for t in keep]

        legs = ("fused", "two_launch", "sweep")
        rounds = {k: [] for k in legs}
        bits, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in legs:
                ms_med, routes[kind], bits[kind] = leg(kind)
                rounds[kind].append(ms_med * 1e3)
        pl.set_plans_path(ctx, 0)
        st = np.frombuffer(bits["two_launch"][4], np.int32)  # the evaluation's status
        out[name] = {"workload": f"{nf} fleets x {M} devices, {len(ks)} k", "routes": routes,
                     "same_bits_fused_two_launch": bits["fused"] == bits["two_launch"],
                     "same_sweep_bits": bits["fused"][:4] == bits["sweep"],
                     "incumbents_feasible": int((st == 0).sum()), "incumbents_infeasible": int((st != 0).sum()),
                     **{f"{k}_event_us": statistics.median(rounds[k]) for k in legs},
                     **{f"{k}_rounds_us": rounds[k] for k in legs}}

    # (c) end to end
    fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(2000 + s, 64)] for s in range(128)]
    old = halda_solve_batch([[DeviceProfile.model_validate(d) for d in synth_fleet(3000 + s, 64)]
                             for s in range(128)], model, kv_bits="4bit")

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
        best = halda_solve_batch(fleets, model, kv_bits="4bit")
        table = fleet_table(fleets, model)
        return best, [pl.evaluate_plan_np(table, model, f, p.k, p.w, p.n, 0.5) for f, p in enumerate(old)]

    a_ms, a_all, a_res = timed(lambda: halda_replace_or_keep_batch(fleets, model, old, kv_bits="4bit"))
    b_ms, b_all, (b_best, b_ev) = timed(by_hand)
    out["c_end_to_end_128x64"] = {
        "halda_replace_or_keep_batch_ms": a_ms, "halda_replace_or_keep_batch_all_ms": a_all,
        "solve_batch_plus_evaluate_plan_np_loop_ms": b_ms, "solve_batch_plus_loop_all_ms": b_all,
        "same_best": [(x.best.k, x.best.w, x.best.n) for x in a_res] == [(x.k, x.w, x.n) for x in b_best],
        "same_feasibility": [x.incumbent.feasible for x in a_res] == [x.feasible for x in b_ev]}
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
