"""A/B of leave-one-out through the sub-fleet entries against the materialised batch.

Leave-one-out of 64 C3 fleets (64 synthetic devices each: 4,096 items of 63 devices), median of 7 warm
calls, wall clock unless noted:
  (a) halda_solve_batch of the 4,096 materialised 63-device lists (the route a caller had before);
  (b) halda_leave_one_out_batch of the 64 fleets;
  (c) by HIP events around one halda_solve_subfleets call on resident device arrays: the fused route
      (halda_sweep_subfleets_kernel) against path 1 (halda_expand_subfleets_kernel + the ordinary sweep).
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/subfleets_ab.py --out profiles/subfleets_ab.json
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
N_FLEETS, M, WARM, REPS = 64, 64, 2, 7


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import halda_leave_one_out_batch, halda_solve_batch
    from distilp_amd.solver import subfleets as sf
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import (BYTE_FIELDS, F64_FIELDS, HaldaFleetResultC, _fleets_struct, fleet_table,
                                           model_struct)
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    fleets = [[DeviceProfile.model_validate(d) for d in synth_fleet(300 + s, M)] for s in range(N_FLEETS)]
    lists = [devs[:i] + devs[i + 1:] for devs in fleets for i in range(M)]

    def timed(fn):
        for _ in range(WARM):
            res = fn()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts, res

    a_ms, a_all, a_res = timed(lambda: halda_solve_batch(lists, model))
    b_ms, b_all, b_res = timed(lambda: halda_leave_one_out_batch(fleets, model))
    same = [r for per in b_res for r in per] == a_res

    # (c) device arrays, HIP events on one stream
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    table = fleet_table(fleets, model)
    arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev)
            for f in ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS}
    fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
    parent, sub_off, sub_idx = sf.leave_one_out_items(table.sizes())
    d = [torch.from_numpy(x).to(dev) for x in (parent, sub_off, sub_idx)]
    n, tot = len(parent), int(sub_off[-1])
    it = sf.HaldaSubfleetsC(n, M - 1, M - 1, *[t.data_ptr() for t in d])
    ks = np.asarray(sorted(k for k in range(1, model.L) if model.L % k == 0), np.int32)
    o = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
         torch.empty(tot, dtype=torch.int32, device=dev), torch.empty(tot, dtype=torch.int32, device=dev)]
    r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
    m = model_struct(model, 1.0)
    stream = torch.cuda.Stream(dev)
    routes, outs = {}, {}
    for name, path in (("fused", 0), ("expand", 1)):
        sf.set_subfleets_path(ctx, path)
        ts = []
        for rep in range(WARM + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = lib.halda_solve_subfleets(ctx.ctx, ctypes.byref(m), ctypes.byref(fs), ctypes.byref(it),
                                           ks.ctypes.data, len(ks), ctypes.byref(r), ctypes.c_void_p(stream.cuda_stream))
            if rc != 0:
                raise RuntimeError(f"halda_solve_subfleets failed ({rc}): {last_error(lib)}")
            e1.record(stream)
            stream.synchronize()
            if rep >= WARM:
                ts.append(e0.elapsed_time(e1))
        routes[name] = {"median_ms": statistics.median(ts), "all_ms": ts}
        outs[name] = [t.cpu().numpy().tobytes() for t in o]
    sf.set_subfleets_path(ctx, 0)
    print(json.dumps({
        "workload": f"leave-one-out of {N_FLEETS} C3 fleets of {M} devices: {n} items of {M - 1} devices",
        "gpu": torch.cuda.get_device_name(0), "reps": REPS,
        "a_halda_solve_batch_ms": a_ms, "a_all_ms": a_all,
        "b_halda_leave_one_out_batch_ms": b_ms, "b_all_ms": b_all, "b_equals_a": same,
        "c_fused_event_ms": routes["fused"]["median_ms"], "c_fused_all_ms": routes["fused"]["all_ms"],
        "c_expand_event_ms": routes["expand"]["median_ms"], "c_expand_all_ms": routes["expand"]["all_ms"],
        "c_same_bits": outs["fused"] == outs["expand"]}))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of the GPU child process, seconds")
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
