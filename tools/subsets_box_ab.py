"""A/B of halda_solve_subsets_boxed's fused routes (candidates formed, priced under every box and reduced on the
device) against (i) the entry's own expansion route (path 1) and (ii) halda_solve_subfleets_boxed over the same
(list, box) items ALREADY materialised on the device, one call per d (uniform list lengths: its best route) -- what
a caller without this entry runs to get the per-candidate values, with the enumeration, the item arrays' PCIe
traffic and the arg-min it still needs left out of its figure. One build.

By HIP events around the calls on resident device arrays, warm, the legs alternated over ROUNDS rounds of REPS calls
each (the median of every round, then the median and the spread of the rounds), on the 80-layer model, D <= 2,
2 boxes (a move box of +-2 layers around the optimum of a perturbed() copy of the table, and an n_max cap):
  a  64 fleets x 64 devices, ks = [1]           (the register route, halda_sweep_subsets_box_kernel);
  b  64 fleets x 16 devices, ks = [2]           (the table route, halda_sweep_subsets_box_tables_kernel);
  c  64 fleets x 16 devices, ks = [1, 2, 4, 5]  (the table route).
And end to end, wall clock: halda_subset_frontier_batch(..., bounds=...) of 8 fleets x 64 devices, D <= 2, against
halda_solve_subfleets_bounded over the host-enumerated lists plus the arg-min in Python.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out, writes it
to a file. A leg that did not run is absent from the line: not measured.

    python tools/subsets_box_ab.py --out profiles/subsets_box_ab.json
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
WARM, REPS, ROUNDS = 2, 7, 5
LEGS = ("fused", "materialised", "expand")
D = 2
IMAX = 2**31 - 1


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import halda_solve_batch, halda_solve_subfleets_bounded, halda_subset_frontier_batch
    from distilp_amd.solver import subfleets_bounded as sb
    from distilp_amd.solver import subsets_bounded as sx
    from distilp_amd.solver._abi import (HaldaBoxesC, HaldaFleetResultC, HaldaSubBoxesC, HaldaSubfleetsC,
                                         HaldaSubsetFrontierC, HaldaSubsetsC)
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.bounds import move_box
    from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, _fleets_struct, fleet_table, model_struct, solve_table
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS, "max_drop": D, "boxes": 2}
    fields = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    m = model_struct(model, 0.5)
    i32, f64 = torch.int32, torch.float64

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    for name, nf, M, ks in (("a_64x64_k1", 64, 64, [1]), ("b_64x16_k2", 64, 16, [2]),
                            ("c_64x16_k1245", 64, 16, [1, 2, 4, 5])):
        table = fleet_table([[DeviceProfile.model_validate(d) for d in synth_fleet(1000 + M + s, M)]
                             for s in range(nf)], model)
        nd, W = table.n_devices, int(model.L) // ks[0]
        karr = np.asarray(ks, np.int32)
        w0 = np.maximum(1, solve_table(table.perturbed(np.random.default_rng(7)), model, ks, 0.5).w.astype(np.int64))
        planes = [np.stack([np.maximum(1, w0 - 2), np.ones(nd, np.int64)]).astype(np.int32),
                  np.stack([w0 + 2, np.full(nd, IMAX)]).astype(np.int32),
                  np.stack([np.full(nd, IMAX), np.full(nd, W // 2)]).astype(np.int32)]  # w_min, w_max, n_max
        arrs = {f: to_dev(getattr(table, f)) for f in fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        pl = [to_dev(p) for p in planes]
        bx = HaldaBoxesC(2, pl[0].data_ptr(), pl[1].data_ptr(), None, pl[2].data_ptr())
        pts = 2 * nf * (D + 1)
        fo = [torch.empty(pts, dtype=i32, device=dev), torch.empty(pts, dtype=f64, device=dev),
              torch.empty(pts, dtype=torch.int64, device=dev), torch.empty(pts, dtype=i32, device=dev)]
        fr = HaldaSubsetFrontierC(*[a.data_ptr() for a in fo])
        sub = HaldaSubsetsC(D, None)
        # leg (ii): per d, every (fleet, box, candidate) as a materialised item
        mat, n_items = [], 0
        for d in range(D + 1):
            kept = np.asarray([[i for i in range(M) if i not in c] for c in itertools.combinations(range(M), d)], np.int32)
            C = len(kept)
            n = nf * 2 * C
            t = {"parent": np.repeat(np.arange(nf, dtype=np.int32), 2 * C),
                 "sub_off": np.arange(n + 1, dtype=np.int64) * (M - d), "sub_idx": np.tile(kept.ravel(), nf * 2),
                 "item_box": np.tile(np.repeat(np.arange(2, dtype=np.int32), C), nf)}
            t = {k: to_dev(v) for k, v in t.items()}
            o = [torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=f64, device=dev),
                 torch.empty(n * (M - d), dtype=i32, device=dev), torch.empty(n * (M - d), dtype=i32, device=dev)]
            mat.append((HaldaSubfleetsC(n, M - d, M - d, t["parent"].data_ptr(), t["sub_off"].data_ptr(),
                                        t["sub_idx"].data_ptr()),
                        HaldaSubBoxesC(2, pl[0].data_ptr(), pl[1].data_ptr(), None, pl[2].data_ptr(),
                                       t["item_box"].data_ptr()),
                        HaldaFleetResultC(*[a.data_ptr() for a in o], None, None, None, None, None), t, o))
            n_items += n

        def call(kind):
            if kind != "materialised":
                return lib.halda_solve_subsets_boxed(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
                                                     karr.ctypes.data, len(ks), ctypes.byref(bx), ctypes.byref(fr), sp)
            for it, sbx, r, _, _ in mat:
                rc = lib.halda_solve_subfleets_boxed(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                     karr.ctypes.data, len(ks), ctypes.byref(sbx), ctypes.byref(r), sp)
                if rc != 0:
                    return rc
            return 0

        def leg(kind):
            sx.set_subsets_boxed_path(ctx, 1 if kind == "expand" else 0)
            ts = []
            for rep in range(WARM + REPS):
                for a in fo:
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
            route = sb.last_subfleets_boxed_route(ctx) if kind == "materialised" else sx.last_subsets_boxed_route(ctx)
            return statistics.median(ts), route, [a.cpu().numpy().copy() for a in fo]

        rounds = {k: [] for k in LEGS}
        res, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for kind in LEGS:
                ms_med, routes[kind], res[kind] = leg(kind)
                rounds[kind].append(ms_med * 1e3)
        sx.set_subsets_boxed_path(ctx, 0)
        med = {k: statistics.median(rounds[k]) for k in LEGS}
        # the materialised leg's own arg-min (NumPy, untimed) against the fused frontier's objectives
        want = np.full((nf, 2, D + 1), np.inf)
        for d, (_, _, _, _, o) in enumerate(mat):
            want[:, :, d] = o[1].cpu().numpy().reshape(nf, 2, -1).min(axis=2)
        got = res["fused"][1].reshape(2, nf, D + 1).transpose(1, 0, 2)
        out[name] = {"workload": f"{nf} fleets x {M} devices, D <= {D}, 2 boxes ({n_items} items), ks = {ks}",
                     "routes": routes, "items": n_items, "feasible_points": int((res["fused"][0] == 0).sum()),
                     "points": pts, "fused_equals_expand_bits": all(a.tobytes() == b.tobytes()
                                                                    for a, b in zip(res["fused"], res["expand"])),
                     "fused_equals_materialised_min": bool((got == want).all()),
                     "materialised_over_fused": med["materialised"] / med["fused"],
                     "expand_over_fused": med["expand"] / med["fused"],
                     **{f"{k}_event_us": med[k] for k in LEGS}, **{f"{k}_rounds_us": rounds[k] for k in LEGS}}
        del mat, arrs, pl

    # end to end: the selection inside a box against the bounded sub-fleet entry over host-enumerated lists
    fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(2000 + s, 64)] for s in range(8)]
    old = halda_solve_batch([[DeviceProfile.model_validate(d) for d in synth_fleet(3000 + s, 64)] for s in range(8)],
                            model, [1], kv_bits="4bit")
    boxes = [move_box(list(p.w), list(p.n), 2, 8) for p in old]
    lists = [(f, [i for i in range(64) if i not in c]) for f in range(8) for d in range(D + 1)
             for c in itertools.combinations(range(64), d)]

    def by_lists():
        res = halda_solve_subfleets_bounded(fleets, model, lists, [boxes], [1], "4bit")
        best = {}
        for (f, kept), r in zip(lists, res):
            at = (f, 64 - len(kept))
            if r is not None and (at not in best or r.obj_value < best[at][1]):
                best[at] = (kept, r.obj_value)
        return [[best.get((f, d), ([], float("inf"))) for d in range(D + 1)] for f in range(8)]

    def keyword():
        return [[(p.kept, p.obj_value) for p in pts]
                for pts in halda_subset_frontier_batch(fleets, model, D, None, [1], kv_bits="4bit", bounds=boxes)]

    def timed(fn, n):
        res = fn()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, res

    legs = {}
    for _ in range(2):  # alternate: the second round's figures are kept
        legs["bounds_keyword"] = timed(keyword, 5)
        legs["by_lists"] = timed(by_lists, 3)
    out["d_end_to_end_8x64_k1"] = {
        "items": len(lists), **{f"{k}_ms": v[0] for k, v in legs.items()}, **{f"{k}_all_ms": v[1] for k, v in legs.items()},
        "by_lists_over_bounds_keyword": legs["by_lists"][0] / legs["bounds_keyword"][0],
        "same_results": legs["bounds_keyword"][2] == legs["by_lists"][2],
        "feasible_points": sum(1 for f in legs["bounds_keyword"][2] for p in f if p[0])}
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
