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

--classes measures halda_solve_partition_classes instead, by the same events, legs and medians: on class-sorted
fleets both routes admit (4 kinds x 4 and 4 x 5 devices) the class route against the mask route -- call (R = 4),
solve (R = 1) and levels (their difference) of each, and whether the raw statuses and values are equal bit for bit
-- and beyond the mask gate the class route alone: 4 x 16 = 64 devices (83,521 codes, global source), 2 x 128 = 256
devices on the 320-layer model, 3 x 8 = 24 devices (LDS source).

    python tools/partition_ab.py --classes --out profiles/partition_classes_ab.json
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
# --classes: name, class sizes, model layers, also the mask route, warm, reps, rounds
CLASS_SHAPES = (("e_4x4", (4, 4, 4, 4), 80, True, 2, 5, 3), ("f_4x5", (5, 5, 5, 5), 80, True, 1, 2, 2),
                ("g_4x16", (16, 16, 16, 16), 80, False, 1, 3, 3), ("h_2x128", (128, 128), 320, False, 1, 3, 3),
                ("i_3x8", (8, 8, 8), 80, False, 2, 5, 3))


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


def child_classes(only) -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import partition as pt
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, _fleets_struct, fleet_table, model_struct
    from distilp_amd.synth import load_model_dict, synth_fleet

    base = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    out = {"gpu": torch.cuda.get_device_name(0)}
    fields = ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    i32, f64 = torch.int32, torch.float64

    for name, counts, L, both, warm, reps, rounds in CLASS_SHAPES:
        if only and name not in only:
            continue
        model = base if L == base.L else base.model_copy(update={"L": L})
        ks = sorted(k for k in range(1, model.L) if model.L % k == 0)
        karr, m = np.asarray(ks, np.int32), model_struct(model, 0.5)
        kinds = [DeviceProfile.model_validate(d) for d in synth_fleet(7700 + len(counts), len(counts))]
        fleet = [kinds[c] for c, n in enumerate(counts) for _ in range(n)]  # class-sorted
        table = fleet_table([fleet], model)
        cls, cnt, _ = pt.device_classes(table, 0)
        assert tuple(cnt.tolist()) == counts
        off = np.ascontiguousarray(table.dev_off, np.int64)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())

        def frontier():
            return [torch.empty(R, dtype=i32, device=dev), torch.empty(R, dtype=f64, device=dev),
                    torch.empty(R * 8, dtype=i32, device=dev), torch.empty(R * 8, dtype=f64, device=dev),
                    torch.empty(R * 8, dtype=i32, device=dev)]

        fr_c, fr_m = frontier(), frontier()
        frc = pt.HaldaPartitionClassesFrontierC(*[t.data_ptr() for t in fr_c])
        frm = pt.HaldaPartitionFrontierC(*[t.data_ptr() for t in fr_m])

        def leg(kind):
            route, groups = kind.split("_")
            r = R if groups == "call" else 1
            ts = []
            for rep in range(warm + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if route == "classes":
                    part = pt.HaldaPartitionClassesC(r, 0, cls.ctypes.data, off.ctypes.data)
                    rc = lib.halda_solve_partition_classes(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
                                                           karr.ctypes.data, len(ks), ctypes.byref(frc), sp)
                else:
                    part = pt.HaldaPartitionC(r, 0)
                    rc = lib.halda_solve_partition(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(part),
                                                   karr.ctypes.data, len(ks), ctypes.byref(frm), sp)
                if rc != 0:
                    raise RuntimeError(f"{kind} failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= warm:
                    ts.append(e0.elapsed_time(e1))
            return statistics.median(ts)

        legs = ("classes_call", "classes_solve") + (("masks_call", "masks_solve") if both else ())
        rnd = {k: [] for k in legs}
        for _ in range(rounds):  # alternate the legs
            for kind in legs:
                rnd[kind].append(leg(kind))
        codes = int(np.prod(np.asarray(counts) + 1))
        rec = {"workload": f"{len(counts)} classes x {counts[0]} devices = {len(fleet)} devices, L = {L}, R = {R}, "
                           f"{codes - 1} codes, {len(ks)} k",
               "source": "lds" if codes <= pt.LDS_CODES else "global",
               **{f"{k}_event_ms": statistics.median(rnd[k]) for k in legs}, **{f"{k}_rounds_ms": rnd[k] for k in legs}}
        rec["classes_levels_event_ms"] = rec["classes_call_event_ms"] - rec["classes_solve_event_ms"]
        leg("classes_call")  # leave the R = 4 points in the frontiers
        rec["classes_status"] = fr_c[0].cpu().numpy().tolist()
        rec["classes_value"] = fr_c[1].cpu().numpy().tolist()
        if both:
            leg("masks_call")
            rec["masks_levels_event_ms"] = rec["masks_call_event_ms"] - rec["masks_solve_event_ms"]
            rec["masks"] = (1 << len(fleet)) - 1
            rec["same_bits"] = bool(fr_c[0].cpu().numpy().tobytes() == fr_m[0].cpu().numpy().tobytes()
                                    and fr_c[1].cpu().numpy().tobytes() == fr_m[1].cpu().numpy().tobytes())
        out[name] = rec
        del arrs
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=float, default=500.0, help="time limit of the GPU child process, seconds")
    ap.add_argument("--only", nargs="+", help="shape names to run (default: all)")
    ap.add_argument("--classes", action="store_true",
                    help="measure halda_solve_partition_classes (against the mask route where both admit the fleet)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        (child_classes if args.classes else child)(args.only)
        return 0
    cmd = ([sys.executable, str(Path(__file__).resolve()), "--child"] + (["--classes"] if args.classes else [])
           + (["--only"] + args.only if args.only else []))
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
