"""A/B of halda_solve_subsets against halda_solve_subfleets of the materialised candidate lists, on one build.

By HIP events around the calls on resident device arrays (the legs alternated over ROUNDS rounds of REPS calls
each: the median of every round, then the median of the rounds), and end to end by wall clock through the
Python entries:
  (a) 64 fleets x 64 devices, max_drop 2 (2,081 candidates each): the selection call on its automatic route
      (fused), the same call forced to expand (halda_set_subsets_path(1)), and the baseline --
      halda_solve_subfleets over all 133,184 lists, their index arrays already on the device, in chunks of
      2^21 listed devices as subfleets.py sends them;
  (b) 64 fleets x 16 devices, max_drop 15 (every non-empty subset, 65,535 each; expansion): the selection call
      and the same baseline over 4,194,240 lists.
The baseline leaves every list's result on the device; bringing them back and reducing them is not counted.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out, writes
it to a file.

    python tools/subsets_ab.py --out profiles/subsets_ab.json
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
SHAPES = (("a_64x64_drop2", 64, 2, 2, 5, 3), ("b_64x16_all", 16, 15, 1, 2, 2))  # name, M, D, warm, reps, rounds
N_FLEETS = 64


def child(only) -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import halda_solve_subfleets, halda_subset_frontier_batch
    from distilp_amd.solver import subfleets as sf
    from distilp_amd.solver import subsets as ss
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaFleetResultC, _fleets_struct, fleet_table,
                                           model_struct)
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    ks = sorted(k for k in range(1, model.L) if model.L % k == 0)
    karr = np.asarray(ks, np.int32)
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    out = {"gpu": torch.cuda.get_device_name(0)}
    fields = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    m = model_struct(model, 0.5)
    i32, f64 = torch.int32, torch.float64

    for name, M, D, warm, reps, rounds in SHAPES:
        if only and name not in only:
            continue
        fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(5000 + 100 * M + s, M)]
                  for s in range(N_FLEETS)]
        table = fleet_table(fleets, model)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nf, P1 = table.n_fleets, D + 1
        fr_t = [torch.empty(nf * P1, dtype=i32, device=dev), torch.empty(nf * P1, dtype=f64, device=dev),
                torch.empty(nf * P1, dtype=torch.int64, device=dev), torch.empty(nf * P1, dtype=i32, device=dev)]
        fr = ss.HaldaSubsetFrontierC(*[t.data_ptr() for t in fr_t])
        sub = ss.HaldaSubsetsC(D, None)
        # the baseline's items: per d (lists of one length), every fleet's candidates, chunked by listed devices
        chunks = []
        for d in range(P1):
            rows = np.asarray([[i for i in range(M) if i not in c] for c in itertools.combinations(range(M), d)],
                              np.int32).reshape(-1, M - d)
            per = max(1, sf.SUBFLEET_CHUNK_DEVICES // (M - d))
            idx = np.tile(rows, (nf, 1))
            par = np.repeat(np.arange(nf, dtype=np.int32), len(rows))
            for a in range(0, len(par), per):
                b = min(a + per, len(par))
                n = b - a
                t = [torch.from_numpy(par[a:b].copy()).to(dev),
                     torch.from_numpy(np.arange(n + 1, dtype=np.int64) * (M - d)).to(dev),
                     torch.from_numpy(idx[a:b].ravel().copy()).to(dev)]
                chunks.append((n, M - d, t))
        n_items = sum(c[0] for c in chunks)
        nmax, dmax = max(c[0] for c in chunks), max(c[0] * c[1] for c in chunks)
        o = [torch.empty(nmax, dtype=i32, device=dev), torch.empty(nmax, dtype=f64, device=dev),
             torch.empty(dmax, dtype=i32, device=dev), torch.empty(dmax, dtype=i32, device=dev)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)

        def leg(kind):
            ss.set_subsets_path(ctx, 1 if kind == "expand" else 0)
            ts = []
            for rep in range(warm + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if kind == "subfleets":
                    for n, ln, t in chunks:
                        it = sf.HaldaSubfleetsC(n, ln, ln, *[x.data_ptr() for x in t])
                        rc = lib.halda_solve_subfleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                       karr.ctypes.data, len(ks), ctypes.byref(r), sp)
                        if rc != 0:
                            raise RuntimeError(f"halda_solve_subfleets failed ({rc}): {last_error(lib)}")
                    route = "subfleets:" + sf.last_subfleets_route(ctx)
                else:
                    rc = lib.halda_solve_subsets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub),
                                                 karr.ctypes.data, len(ks), ctypes.byref(fr), sp)
                    if rc != 0:
                        raise RuntimeError(f"halda_solve_subsets failed ({rc}): {last_error(lib)}")
                    route = ss.last_subsets_route(ctx)
                e1.record(stream)
                stream.synchronize()
                if rep >= warm:
                    ts.append(e0.elapsed_time(e1))
            bits = [t.cpu().numpy().tobytes() for t in fr_t] if kind != "subfleets" else None
            return statistics.median(ts), route, bits

        legs = ("auto", "expand", "subfleets")
        rnd = {k: [] for k in legs}
        routes, bits = {}, {}
        for _ in range(rounds):  # alternate the legs
            for kind in legs:
                ms, routes[kind], bits[kind] = leg(kind)
                rnd[kind].append(ms)
        ss.set_subsets_path(ctx, 0)
        rec = {"workload": f"{nf} fleets x {M} devices, max_drop {D}, {n_items} candidates, {len(ks)} k",
               "baseline_chunks": len(chunks), "routes": routes, "same_bits_auto_expand": bits["auto"] == bits["expand"],
               **{f"{k}_event_ms": statistics.median(rnd[k]) for k in legs}, **{f"{k}_rounds_ms": rnd[k] for k in legs}}
        rec["subfleets_over_auto"] = rec["subfleets_event_ms"] / rec["auto_event_ms"]
        rec["expand_over_auto"] = rec["expand_event_ms"] / rec["auto_event_ms"]
        if M == 64:  # end to end through the Python entries, on 8 of the fleets (16,648 lists for the baseline)
            few = fleets[:8]
            items = [(f, [i for i in range(M) if i not in c]) for f in range(len(few)) for d in range(P1)
                     for c in itertools.combinations(range(M), d)]

            def wall(fn):
                fn()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return statistics.median(ts)

            rec["end_to_end_8_fleets"] = {
                "halda_subset_frontier_batch_ms": wall(lambda: halda_subset_frontier_batch(few, model, D)),
                "halda_solve_subfleets_of_every_list_ms": wall(lambda: halda_solve_subfleets(few, model, items)),
                "lists": len(items)}
        out[name] = rec
        del chunks, o, arrs
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=float, default=500.0, help="time limit of the GPU child process, seconds")
    ap.add_argument("--only", nargs="+", help="shape names to run (default: all)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.only)
        return 0
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child"] + (["--only"] + args.only if args.only else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
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
