"""A/B of halda_solve_fleets_boxes' fused routes (one launch over every box) against its loop route (one
halda_solve_fleets_boxed call per box, halda_set_boxes_path(ctx, 1)), one build.

By HIP events around one call on resident device arrays (best_k, obj_value, w, n), warm, the legs alternated over
ROUNDS rounds of REPS calls each (the median of every round, then the median and the spread of the rounds), on the
80-layer model:
  a  1 fleet x 16 devices x 64 boxes, ks = [2]: the ladder w_max = w0 + j around the optimum of a perturbed() copy
     of the table (the table route, halda_sweep_boxes_tables_kernel);
  b  256 fleets x 64 devices x 8 boxes, ks = [1]: the move boxes +-D, D = 0 .. 7, around such an optimum (the
     register route, halda_sweep_boxes_kernel).
The loop route's figure includes its read-back of dev_off[n_fleets] (one stream wait per call), as a caller of the
device entry pays it. And end to end, wall clock: halda_reload_frontier of one 16-device fleet (one packing, one
call) against halda_solve_bounded_batch([devs] * n, ..., route="tables") over the same boxes (n packings of the
fleet in one table, one call).
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out, writes it
to a file.

    python tools/boxes_ab.py --out profiles/boxes_ab.json
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
LEGS = ("fused", "loop")
IMAX = 2**31 - 1


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import boxes as bx
    from distilp_amd.solver import halda_reload_frontier, halda_solve_batch, halda_solve_bounded_batch
    from distilp_amd.solver._abi import HaldaBoxesC, HaldaFleetResultC
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.bounds import last_bounds_route
    from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, _fleets_struct, fleet_table, model_struct, solve_table
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS}
    fields = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS

    def ladder(w0, nb):  # box j: every device may gain j layers
        return (None, np.stack([w0 + j for j in range(nb)]).astype(np.int32))

    def moves(w0, nb):  # box D: at most D layers per device away from w0
        return (np.stack([np.maximum(1, w0 - D) for D in range(nb)]).astype(np.int32),
                np.stack([w0 + D for D in range(nb)]).astype(np.int32))

    for name, nf, M, nb, ks, make in (("a_1x16_64boxes_k2", 1, 16, 64, [2], ladder),
                                      ("b_256x64_8boxes_k1", 256, 64, 8, [1], moves)):
        table = fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(1000 + M + s, M)]
                             for s in range(nf)], model)
        karr = np.asarray(ks, np.int32)
        inc = solve_table(table.perturbed(np.random.default_rng(7)), model, ks, 0.5)
        planes = make(inc.w.astype(np.int64), nb)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nd = table.n_devices
        i32, f64 = torch.int32, torch.float64
        o = [torch.empty(nb * nf, dtype=i32, device=dev), torch.empty(nb * nf, dtype=f64, device=dev),
             torch.empty(nb * nd, dtype=i32, device=dev), torch.empty(nb * nd, dtype=i32, device=dev)]
        bt = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
        bs = HaldaBoxesC(nb, *[None if t is None else t.data_ptr() for t in bt], None, None)
        m = model_struct(model, 0.5)

        def leg(kind):
            bx.set_boxes_path(ctx, 1 if kind == "loop" else 0)
            ts = []
            for rep in range(WARM + REPS):
                for t in o:
                    t.fill_(-7)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = lib.halda_solve_fleets_boxes(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), karr.ctypes.data, len(ks),
                                                  ctypes.byref(bs), ctypes.byref(r), ctypes.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            route = bx.last_boxes_route(ctx)
            if kind == "loop":
                route += " of " + last_bounds_route(ctx)
            return statistics.median(ts), route, [t.cpu().numpy().copy() for t in o]

        rounds = {k: [] for k in LEGS}
        res, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in LEGS:
                ms_med, routes[kind], res[kind] = leg(kind)
                rounds[kind].append(ms_med * 1e3)
        bx.set_boxes_path(ctx, 0)
        med = {k: statistics.median(rounds[k]) for k in LEGS}
        out[name] = {"workload": f"{nf} fleets x {M} devices x {nb} boxes, ks = {ks}", "routes": routes,
                     "same_bits": all(a.tobytes() == b.tobytes() for a, b in zip(res["fused"], res["loop"])),
                     "feasible": int((res["fused"][0] > 0).sum()), "slices": nb * nf,
                     "loop_over_fused": med["loop"] / med["fused"],
                     **{f"{k}_event_us": med[k] for k in LEGS}, **{f"{k}_rounds_us": rounds[k] for k in LEGS}}

    # end to end: the reload frontier of one 16-device fleet against the same boxes through the per-fleet entry
    devs = [DeviceProfile.model_validate(d) for d in synth_fleet(2000, 16)]
    old = halda_solve_batch([[DeviceProfile.model_validate(d) for d in synth_fleet(3000, 16)]], model, [2],
                            kv_bits="4bit")[0]
    inc = (2, list(old.w), list(old.n))
    pts = halda_reload_frontier(devs, model, inc, kv_bits="4bit")
    boxes = [(None, [a + c for a, c in zip(old.w, p.caps)]) for p in pts] + [None]

    def timed(fn):
        for _ in range(2):
            res = fn()
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, res

    legs = {}
    for _ in range(2):  # alternate: the second round's figures are kept
        legs["frontier"] = timed(lambda: halda_reload_frontier(devs, model, inc, kv_bits="4bit"))
        legs["per_fleet"] = timed(lambda: halda_solve_bounded_batch([devs] * len(boxes), model, boxes, [2],
                                                                    kv_bits="4bit", route="tables"))
    # the frontier's points are a running minimum of the per-box answers
    best, same = None, True
    for p, r in zip(legs["frontier"][2], legs["per_fleet"][2]):
        if r is not None and (best is None or r.obj_value < best.obj_value):
            best = r
        same = same and best is not None and p.plan is not None and (p.plan.w, p.plan.n, p.obj_value) == (best.w, best.n, best.obj_value)
    out["c_end_to_end_reload_frontier_1x16_k2"] = {
        "boxes": len(boxes), "frontier_ms": legs["frontier"][0], "frontier_all_ms": legs["frontier"][1],
        "per_fleet_ms": legs["per_fleet"][0], "per_fleet_all_ms": legs["per_fleet"][1],
        "per_fleet_over_frontier": legs["per_fleet"][0] / legs["frontier"][0], "same_results": same}
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
