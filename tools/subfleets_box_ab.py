"""A/B of halda_solve_subfleets_boxed's fused routes (one launch that gathers fields and bounds from the parent
table) against halda_solve_fleets_boxed on the same lists ALREADY materialised on the device with their bounds
gathered (bounds path 3: the entry a caller had before, with the re-packing and the PCIe traffic it needs left out
of its figure), and against the entry's own expansion route (path 1: the two gather launches a caller without
the fused kernels pays on the device, then that same boxed launch), one build.

By HIP events around one call on resident device arrays (best_k, obj_value, w, n), warm, the legs alternated over
ROUNDS rounds of REPS calls each (the median of every round, then the median and the spread of the rounds), on the
80-layer model, every leave-one-out list of every fleet under a move box of +-2 layers around the optimum of a
perturbed() copy of the table:
  a  64 fleets x 64 devices, ks = [1]           (the register route, halda_sweep_subfleets_box_kernel);
  b  256 fleets x 16 devices, ks = [2]          (the table route, halda_sweep_subfleets_box_tables_kernel);
  c  256 fleets x 16 devices, ks = [1, 2, 4, 5] (the table route).
And end to end, wall clock: halda_leave_one_out_batch(..., bounds=...) of 32 fleets x 16 devices against a Python
loop of halda_solve_bounded_batch(route="tables") over each fleet's materialised lists.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out, writes it
to a file.

    python tools/subfleets_box_ab.py --out profiles/subfleets_box_ab.json
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
LEGS = ("fused", "materialised", "expand")


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import halda_leave_one_out_batch, halda_solve_batch, halda_solve_bounded_batch
    from distilp_amd.solver import subfleets_bounded as sb
    from distilp_amd.solver._abi import HaldaBoxC, HaldaFleetResultC, HaldaSubBoxesC, HaldaSubfleetsC
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.bounds import last_bounds_route, move_bounds, set_bounds_path
    from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, _fleets_struct, fleet_table, model_struct, solve_table
    from distilp_amd.solver.subfleets import gather_table, leave_one_out_items
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS}
    fields = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    m = model_struct(model, 0.5)

    def resident(table):
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in fields}
        return _fleets_struct(table, lambda f: arrs[f].data_ptr()), arrs

    for name, nf, M, ks in (("a_64x64_k1", 64, 64, [1]), ("b_256x16_k2", 256, 16, [2]),
                            ("c_256x16_k1245", 256, 16, [1, 2, 4, 5])):
        table = fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(1000 + M + s, M)]
                             for s in range(nf)], model)
        karr = np.asarray(ks, np.int32)
        w0 = np.maximum(1, solve_table(table.perturbed(np.random.default_rng(7)), model, ks, 0.5).w.astype(np.int64))
        lo, hi = np.maximum(1, w0 - 2).astype(np.int32), (w0 + 2).astype(np.int32)
        parent, sub_off, sub_idx = leave_one_out_items([M] * nf)
        n, tot = len(parent), int(sub_off[-1])
        g = np.repeat(table.dev_off[parent.astype(np.int64)], np.diff(sub_off)) + sub_idx
        fs, keep_a = resident(table)
        gs, keep_b = resident(gather_table(table, parent, sub_off, sub_idx))
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
             for k, v in (("parent", parent), ("sub_off", sub_off), ("sub_idx", sub_idx), ("lo", lo), ("hi", hi),
                          ("glo", lo[g]), ("ghi", hi[g]))}
        i32, f64 = torch.int32, torch.float64
        o = [torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=f64, device=dev),
             torch.empty(tot, dtype=i32, device=dev), torch.empty(tot, dtype=i32, device=dev)]
        r = HaldaFleetResultC(*[a.data_ptr() for a in o], None, None, None, None, None)
        it = HaldaSubfleetsC(n, M - 1, M - 1, t["parent"].data_ptr(), t["sub_off"].data_ptr(), t["sub_idx"].data_ptr())
        sbx = HaldaSubBoxesC(1, t["lo"].data_ptr(), t["hi"].data_ptr(), None, None, None)
        box = HaldaBoxC(t["glo"].data_ptr(), t["ghi"].data_ptr(), None, None)
        sp = ctypes.c_void_p(stream.cuda_stream)

        def call(kind):
            if kind != "materialised":
                return lib.halda_solve_subfleets_boxed(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                       karr.ctypes.data, len(ks), ctypes.byref(sbx), ctypes.byref(r), sp)
            return lib.halda_solve_fleets_boxed(ctx.ctx, ctypes.byref(m), ctypes.byref(gs), karr.ctypes.data, len(ks),
                                                ctypes.byref(box), ctypes.byref(r), sp)

        def leg(kind):
            set_bounds_path(ctx, 3 if kind == "materialised" else 0)
            sb.set_subfleets_boxed_path(ctx, 1 if kind == "expand" else 0)
            ts = []
            for rep in range(WARM + REPS):
                for a in o:
                    a.fill_(-7)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = call(kind)
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            route = last_bounds_route(ctx) if kind == "materialised" else sb.last_subfleets_boxed_route(ctx)
            return statistics.median(ts), route, [a.cpu().numpy().copy() for a in o]

        rounds = {k: [] for k in LEGS}
        res, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in LEGS:
                ms_med, routes[kind], res[kind] = leg(kind)
                rounds[kind].append(ms_med * 1e3)
        set_bounds_path(ctx, 0)
        sb.set_subfleets_boxed_path(ctx, 0)
        med = {k: statistics.median(rounds[k]) for k in LEGS}
        out[name] = {"workload": f"leave-one-out of {nf} fleets x {M} devices ({n} items), ks = {ks}, box +-2",
                     "routes": routes, "feasible": int((res["fused"][0] > 0).sum()), "items": n,
                     "same_bits": all(a.tobytes() == b.tobytes() for a, b in zip(res["fused"], res["materialised"])),
                     "materialised_over_fused": med["materialised"] / med["fused"],
                     "expand_over_fused": med["expand"] / med["fused"],
                     **{f"{k}_event_us": med[k] for k in LEGS}, **{f"{k}_rounds_us": rounds[k] for k in LEGS}}
        del keep_a, keep_b

    # end to end: leave-one-out inside a box against a loop of bounded batches over materialised lists
    fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(2000 + s, 16)] for s in range(32)]
    old = halda_solve_batch([[DeviceProfile.model_validate(d) for d in synth_fleet(3000 + s, 16)] for s in range(32)],
                            model, [2], kv_bits="4bit")
    boxes = [move_bounds(list(p.w), 2) for p in old]

    def loop():
        res = []
        for devs, (lo, hi) in zip(fleets, boxes):
            keeps = [[j for j in range(16) if j != i] for i in range(16)]
            res.append(halda_solve_bounded_batch([[devs[j] for j in k] for k in keeps], model,
                                                 [([lo[j] for j in k], [hi[j] for j in k]) for k in keeps], [2],
                                                 kv_bits="4bit", route="tables"))
        return res

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
        legs["bounds_keyword"] = timed(lambda: halda_leave_one_out_batch(fleets, model, [2], kv_bits="4bit", bounds=boxes))
        legs["loop"] = timed(loop)

    def key(x):
        return None if x is None else (x.k, list(x.w), list(x.n), x.obj_value)

    out["d_end_to_end_leave_one_out_32x16_k2"] = {
        "items": 32 * 16, **{f"{k}_ms": v[0] for k, v in legs.items()}, **{f"{k}_all_ms": v[1] for k, v in legs.items()},
        "loop_over_bounds_keyword": legs["loop"][0] / legs["bounds_keyword"][0],
        "same_results": [[key(x) for x in f] for f in legs["bounds_keyword"][2]] == [[key(x) for x in f] for f in legs["loop"][2]]}
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
