"""Timing of the rank routes of device selection and scale-in (halda_solve_subsets_wide,
halda_solve_change_subsets_wide; route="wide"), beside what there is without them.

Two shapes, every fleet holding its own optimum at k = 1, d <= 2 devices dropped:
  a_1x100   one fleet of 100 devices on the model at 160 layers (W = 160), selection and scale-in at P = 4: 5,051
            candidates. No other route takes it; the baseline is the host enumeration of the same lists through
            halda_solve_subfleets / halda_failover_frontiers(route="wide"), end to end. The wide calls are also
            timed on the device.
  b_64x16   64 fleets of 16 devices on the 80-layer model, selection and scale-in at P = 4: the wave route on the
            same call, i.e. the cost of ranks against masks inside the wave gate.
Device times are HIP events, warm, on resident device arrays, the legs alternated over ROUNDS rounds of REPS calls
(the median of every round, then the median of the rounds); end-to-end times are the wall clock from Python
objects to Python objects, REPS_E2E calls after one warm call. The GPU work is one child process under a time
limit; the parent prints one JSON line and, with --out, writes it.

    python tools/select_wide_ab.py --out profiles/select_wide_ab.json
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
WARM, REPS, ROUNDS, REPS_E2E = 2, 5, 3, 2
K, D, P = 1, 2, 4


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import _abi as abi
    from distilp_amd.solver import change as ch
    from distilp_amd.solver import scale as sc
    from distilp_amd.solver import subsets as ss
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, _fleets_struct, fleet_table, model_struct, solve_table
    from distilp_amd.solver.subfleets import halda_solve_subfleets
    from distilp_amd.synth import load_model_dict, synth_fleet

    base = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    stream = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS, "reps_end_to_end": REPS_E2E, "k": K,
           "max_drop": D, "max_p": P}
    fields = ("os_class", "flags") + F64_FIELDS + BYTE_FIELDS
    i32, f64 = torch.int32, torch.float64
    ks = np.asarray([K], np.int32)

    def events(call):
        ts = []
        for rep in range(WARM + REPS):
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = call()
            e1.record(stream)
            stream.synchronize()
            if rc != 0:
                raise RuntimeError(f"call failed ({rc}): {last_error(lib)}")
            if rep >= WARM:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts)

    def wall(fn):
        fn()
        ts, got = [], None
        for _ in range(REPS_E2E):
            t0 = time.perf_counter()
            got = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), got

    for name, nf, M, L in (("a_1x100", 1, 100, 160), ("b_64x16", 64, 16, 80)):
        model = base.model_copy(update={"L": L})
        fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(1000 + M + s, M)] for s in range(nf)]
        table = fleet_table(fleets, model)
        inc = solve_table(table, model, [K], 0.5)
        assert (inc.best_k == K).all()
        w_all = inc.w.astype(np.int32)
        off = [int(v) for v in table.dev_off[:nf + 1]]
        incs = [(K, w_all[off[f]:off[f + 1]].tolist(), inc.n[off[f]:off[f + 1]].tolist()) for f in range(nf)]
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev) for f in ("dev_off",) + fields}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        m = model_struct(model, 0.5)
        tw0 = torch.from_numpy(w_all).to(dev)
        sel_pts, pts = nf * (D + 1), nf * (D + 1) * (P + 1)
        t = lambda n, dt=i32: torch.empty(n, dtype=dt, device=dev)  # noqa: E731
        sel_wide = [t(sel_pts), t(sel_pts, f64), t(sel_pts * D), t(sel_pts)]
        sel_wave = [t(sel_pts), t(sel_pts, f64), t(sel_pts, torch.int64), t(sel_pts)]
        sc_wide = [t(pts), t(pts, f64), t(pts * D), t(pts), t(pts), t(pts * 256), t(pts * 256)]
        sc_wave = [t(pts), t(pts, f64), t(pts, torch.int64), t(pts), t(pts), t(pts * 64), t(pts * 64)]
        structs = {
            "select_wide": (abi.HaldaSubsetsWideC(D, None), abi.HaldaSubsetFrontierWideC(*[x.data_ptr() for x in sel_wide])),
            "select_wave": (abi.HaldaSubsetsC(D, None), abi.HaldaSubsetFrontierC(*[x.data_ptr() for x in sel_wave])),
            "scale_wide": (abi.HaldaChangeSubsetsWideC(tw0.data_ptr(), None, None, 0, D, P, None),
                           abi.HaldaChangeSubsetFrontierWideC(*[x.data_ptr() for x in sc_wide])),
            "scale_wave": (abi.HaldaChangeSubsetsC(tw0.data_ptr(), None, None, 0, D, P, None),
                           abi.HaldaChangeSubsetFrontierC(*[x.data_ptr() for x in sc_wave]))}

        def call(leg):
            sub, fr = structs[leg]
            if leg.startswith("select"):
                fn = lib.halda_solve_subsets_wide if leg.endswith("wide") else lib.halda_solve_subsets
                return fn(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(sub), ks.ctypes.data, 1,
                          ctypes.byref(fr), sp)
            fn = lib.halda_solve_change_subsets_wide if leg.endswith("wide") else lib.halda_solve_change_subsets
            return fn(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), K, ctypes.byref(sub), ctypes.byref(fr), sp)

        legs = [g for g in structs if g.endswith("wide") or M <= 64]
        rounds = {g: [] for g in legs}
        for _ in range(ROUNDS):
            for g in legs:
                rounds[g].append(events(lambda g=g: call(g)))
        rec = {"workload": f"{nf} fleets x {M} devices, L = {L}, d <= {D}, P = {P}: "
                           f"{nf * ss.subsets_count(M, D)} candidate lists",
               **{f"{g}_event_us": statistics.median(rounds[g]) for g in legs},
               **{f"{g}_rounds_us": rounds[g] for g in legs}}
        if M <= 64:
            rec["select_wide_over_wave_events"] = rec["select_wide_event_us"] / rec["select_wave_event_us"]
            rec["scale_wide_over_wave_events"] = rec["scale_wide_event_us"] / rec["scale_wave_event_us"]
            rec["select_bits_equal"] = bool(torch.equal(sel_wide[1].view(torch.int64), sel_wave[1].view(torch.int64)))
            rec["scale_bits_equal"] = bool(torch.equal(sc_wide[1].view(torch.int64), sc_wave[1].view(torch.int64)))
            for what, fn in (("select", lambda r: ss.halda_subset_frontier_batch(fleets, model, D, k_candidates=[K],
                                                                                 kv_bits="4bit", route=r)),
                             ("scale", lambda r: sc.halda_scale_in_frontier_batch(fleets, model, incs, D, P,
                                                                                  kv_bits="4bit", route=r))):
                ww, a = wall(lambda: fn("wave"))
                wd, b = wall(lambda: fn("wide"))
                rec[f"{what}_wave_end_to_end_ms"], rec[f"{what}_wide_end_to_end_ms"] = ww, wd
                rec[f"{what}_end_to_end_equal"] = a == b
        else:
            devs, lost = fleets[0], [c for d in range(D + 1) for c in itertools.combinations(range(M), d)]
            kept = [[i for i in range(M) if i not in set(c)] for c in lost]

            def by_lists_select():
                res = halda_solve_subfleets([devs], model, [(0, kp) for kp in kept], [K], kv_bits="4bit")
                best = [None] * (D + 1)
                for c, r in zip(lost, res):
                    if r is not None and (best[len(c)] is None or r.obj_value < best[len(c)][1].obj_value):
                        best[len(c)] = (c, r)
                return best

            def by_lists_scale():
                frs = ch.halda_failover_frontiers(devs, model, incs[0], P, lost[1:], "4bit", route="wide")
                rows = [[None] * (P + 1) for _ in range(D + 1)]
                for c, fr in zip(lost[1:], frs):
                    for p, pt in enumerate(fr):
                        cur = rows[len(c)][p]
                        if pt.plan is not None and (cur is None or pt.obj_value < cur[1].obj_value):
                            rows[len(c)][p] = (c, pt)
                return rows

            ws, a = wall(lambda: ss.halda_subset_frontier(devs, model, D, k_candidates=[K], kv_bits="4bit", route="wide"))
            wl, b = wall(by_lists_select)
            rec.update(select_wide_end_to_end_ms=ws, select_lists_end_to_end_ms=wl, select_end_to_end_speedup=wl / ws,
                       select_agrees=all(b[d] is not None and list(b[d][0]) == a[d].dropped and
                                         b[d][1].obj_value == a[d].obj_value for d in range(D + 1)))
            ws, a = wall(lambda: sc.halda_scale_in_frontier(devs, model, incs[0], D, P, kv_bits="4bit", route="wide"))
            wl, b = wall(by_lists_scale)
            rec.update(scale_wide_end_to_end_ms=ws, scale_lists_end_to_end_ms=wl, scale_end_to_end_speedup=wl / ws,
                       scale_agrees=all((b[d][p] is None) == (a[d][p].point.plan is None) and
                                        (b[d][p] is None or b[d][p][1].obj_value == a[d][p].point.obj_value)
                                        for d in range(1, D + 1) for p in range(P + 1)))
        out[name] = rec
        print(name, json.dumps(rec), file=sys.stderr, flush=True)
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
