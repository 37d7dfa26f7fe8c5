"""A/B of halda_solve_partition against its own host alternative, on one build.

By HIP events around the calls on resident device arrays (the legs alternated over ROUNDS rounds of REPS calls each:
the median of every round, then the median of the rounds):
  partition    halda_solve_partition at R = 4, criterion max;
  solve_only   the same call at R = 1 -- every mask solved and traced, no level launch -- so that
               partition - solve_only is the time of the level kernels (levels 2, 3 and the full mask of level 4);
  subfleets    the alternative's device half: halda_solve_subfleets over every mask's list, the index arrays already
               on the device, in chunks of 2^21 listed devices as subfleets.py sends them.
The alternative's host half, the recurrence in NumPy over the values brought back (one vectorised minimum per S), is
timed by wall clock where it is tractable (fleets of at most 13 devices). End to end by wall clock through the Python
entries on the first shape: halda_partition_frontier_batch against halda_solve_subfleets of every list plus that
recurrence. Shapes: 64 fleets x 8 devices, 8 x 13 (LDS source), 1 x 16 and 1 x 20 (global source).
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out, writes it to a
file.

    python tools/partition_ab.py --out profiles/partition_ab.json
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
SHAPES = (("a_64x8", 64, 8, 2, 5, 3), ("b_8x13", 8, 13, 1, 3, 3), ("c_1x16", 1, 16, 1, 3, 3),
          ("d_1x20", 1, 20, 1, 2, 2))  # name, fleets, M, warm, reps, rounds
R = 4


def recurrence(val, M, R):
    """best_r of the full mask, r = 1 .. R, criterion max, over val[1 .. 2^M - 1] (val[0] unused)."""
    import numpy as np

    full, prev, out = (1 << M) - 1, val, [val[-1]]
    subs = {0: np.zeros(1, np.int64)}
    for S in range(1, full + 1):  # the submasks of S, ascending
        low = S & -S
        subs[S] = np.concatenate([subs[S ^ low], subs[S ^ low] | low])
    for r in range(2, R + 1):
        cur = np.full(full + 1, np.inf)
        for S in ([full] if r == R else range(1, full + 1)):
            T = subs[S][1:-1]
            T = T[(T & (S & -S)) != 0]
            if len(T) and bin(S).count("1") >= r:
                cur[S] = np.min(np.maximum(val[T], prev[S ^ T]))
        out.append(cur[full])
        prev = cur
    return out


def child(only) -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import halda_partition_frontier_batch, halda_solve_subfleets
    from distilp_amd.solver import partition as pt
    from distilp_amd.solver import subfleets as sf
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

    for name, nf, M, warm, reps, rounds in SHAPES:
        if only and name not in only:
            continue
        fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(7000 + 100 * M + s, M)] for s in range(nf)]
        table = fleet_table(fleets, model)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        fr_t = [torch.empty(nf * R, dtype=i32, device=dev), torch.empty(nf * R, dtype=f64, device=dev),
                torch.empty(nf * R * 8, dtype=i32, device=dev), torch.empty(nf * R * 8, dtype=f64, device=dev),
                torch.empty(nf * R * 8, dtype=i32, device=dev)]
        fr = pt.HaldaPartitionFrontierC(*[t.data_ptr() for t in fr_t])
        # the baseline's items: every mask of every fleet, chunked by listed devices
        masks = np.arange(1, 1 << M, dtype=np.int64)
        bits = (masks[:, None] >> np.arange(M)) & 1
        lens = bits.sum(axis=1)
        idx = np.nonzero(bits)[1].astype(np.int32)
        lens_all, idx_all = np.tile(lens, nf), np.tile(idx, nf)
        par_all = np.repeat(np.arange(nf, dtype=np.int32), len(masks))
        off_all = np.concatenate([[0], np.cumsum(lens_all)])
        chunks = []
        for a, b in sf.plan_chunks(lens_all, sf.SUBFLEET_CHUNK_DEVICES):
            lo, hi = int(off_all[a]), int(off_all[b])
            t = [torch.from_numpy(par_all[a:b].copy()).to(dev), torch.from_numpy(off_all[a:b + 1] - lo).to(dev),
                 torch.from_numpy(idx_all[lo:hi].copy()).to(dev)]
            chunks.append((b - a, int(lens_all[a:b].min()), int(lens_all[a:b].max()), hi - lo, t))
        dmax = max(c[3] for c in chunks)
        o = [torch.empty(len(par_all), dtype=i32, device=dev), torch.empty(len(par_all), dtype=f64, device=dev),
             torch.empty(dmax, dtype=i32, device=dev), torch.empty(dmax, dtype=i32, device=dev)]

        def leg(kind):
            ts = []
            for rep in range(warm + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if kind == "subfleets":
                    at = 0
                    for n, lmin, lmax, _, t in chunks:
                        it = sf.HaldaSubfleetsC(n, lmin, lmax, *[x.data_ptr() for x in t])
                        r = HaldaFleetResultC(o[0].data_ptr() + 4 * at, o[1].data_ptr() + 8 * at, o[2].data_ptr(),
                                              o[3].data_ptr(), None, None, None, None, None)
                        rc = lib.halda_solve_subfleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                                       karr.ctypes.data, len(ks), ctypes.byref(r), sp)
                        if rc != 0:
                            raise RuntimeError(f"halda_solve_subfleets failed ({rc}): {last_error(lib)}")
                        at += n
                else:
                    part = pt.HaldaPartitionC(R if kind == "partition" else 1, 0)
                    rc = lib.halda_solve_partition(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
                                                   karr.ctypes.data, len(ks), ctypes.byref(fr), sp)
                    if rc != 0:
                        raise RuntimeError(f"halda_solve_partition failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= warm:
                    ts.append(e0.elapsed_time(e1))
            return statistics.median(ts)

        legs = ("partition", "solve_only", "subfleets")
        rnd = {k: [] for k in legs}
        for _ in range(rounds):  # alternate the legs
            for kind in legs:
                rnd[kind].append(leg(kind))
        leg("subfleets")  # leave every mask's value in o, then the R = 4 points in fr_t, for the check below
        leg("partition")
        values = fr_t[1].cpu().numpy().reshape(nf, R)
        rec = {"workload": f"{nf} fleets x {M} devices, R = {R}, {nf * len(masks)} masks, {len(ks)} k",
               "source": "lds" if M <= pt.LDS_DEVICES else "global", "baseline_chunks": len(chunks),
               **{f"{k}_event_ms": statistics.median(rnd[k]) for k in legs}, **{f"{k}_rounds_ms": rnd[k] for k in legs}}
        rec["levels_event_ms"] = rec["partition_event_ms"] - rec["solve_only_event_ms"]
        if M <= pt.LDS_DEVICES:  # the alternative's host half, and that both halves give the call's values
            val = np.concatenate([[np.inf], o[1][:len(masks)].cpu().numpy()])
            t0 = time.perf_counter()
            want = recurrence(val, M, R)
            rec["numpy_recurrence_ms_per_fleet"] = (time.perf_counter() - t0) * 1e3
            rec["alternative_ms"] = rec["subfleets_event_ms"] + nf * rec["numpy_recurrence_ms_per_fleet"]
            rec["same_values"] = bool(np.array_equal(np.asarray(want), values[0]))
        if name == "a_64x8":  # end to end through the Python entries, on 8 of the fleets
            few = fleets[:8]
            items = [(f, pt.mask_devices(int(s))) for f in range(len(few)) for s in masks]

            def loop():
                res = halda_solve_subfleets(few, model, items, kv_bits="4bit")
                for f in range(len(few)):
                    v = np.asarray([np.inf] + [np.inf if x is None else x.obj_value
                                               for x in res[f * len(masks):(f + 1) * len(masks)]])
                    recurrence(v, M, R)

            def wall(fn):
                fn()
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return statistics.median(ts)

            rec["end_to_end_8_fleets"] = {
                "halda_partition_frontier_batch_ms": wall(lambda: halda_partition_frontier_batch(few, model, R,
                                                                                                 kv_bits="4bit")),
                "python_loop_ms": wall(loop), "lists": len(items)}
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
