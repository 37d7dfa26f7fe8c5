"""A/B of halda_solve_variants: the fused route against the per-variant loop, on one build.

Two cases, by HIP events around one halda_solve_variants call on resident device arrays (best_k, obj_value,
w, n only), the two legs alternated over ROUNDS rounds of REPS calls each (the median of every round, then
the median and the spread of the rounds):
  (1) one 4-device fixture fleet (tests/golden/synthetic_M4.json, fleet 0) x 48 variants
      (16 n_kv x 3 KV precisions): the table route, halda_sweep_tables_variants_kernel;
  (2) 256 C3 fleets (64 synthetic devices each) x 8 variants: the register route,
      halda_sweep_variants_kernel.
And end to end, wall clock: halda_solve_variants against a Python loop of halda_solve_batch, same cases.
The GPU work is one child process under a time limit; the parent prints one JSON line and, with --out,
writes it to a file.

    python tools/variants_ab.py --out profiles/variants_ab.json
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


def child() -> None:
    sys.path.insert(0, str(REPO))
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import DeviceProfile, ModelProfileSplit
    from distilp_amd.solver import halda_solve_batch, halda_solve_variants, model_grid
    from distilp_amd.solver import variants as va
    from distilp_amd.solver._libhalda import get_context, last_error
    from distilp_amd.solver.fleets import BYTE_FIELDS, F64_FIELDS, HaldaFleetResultC, _fleets_struct, fleet_table
    from distilp_amd.synth import load_model_dict, synth_fleet

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    m4 = json.loads((REPO / "tests" / "golden" / "synthetic_M4.json").read_text())["fleets"][0]["devices"]
    cases = {
        "fixture4_x48": ([[DeviceProfile.model_validate(d) for d in m4]],
                         model_grid(model, ("4bit", "8bit", "fp16"), [1 << e for e in range(7, 23)])),
        "c3_256_x8": ([[DeviceProfile.model_validate(d) for d in synth_fleet(300 + s, 64)] for s in range(256)],
                      model_grid(model, ("4bit", "fp16"), [512, 4096, 65536, 1 << 20])),
    }
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    lib = ctx.lib
    ks = np.asarray(sorted(k for k in range(1, model.L) if model.L % k == 0), np.int32)
    stream = torch.cuda.Stream(dev)
    out = {"gpu": torch.cuda.get_device_name(0), "reps": REPS, "rounds": ROUNDS}
    for name, (fleets, variants) in cases.items():
        table = fleet_table(fleets, model)
        arrs = {f: torch.from_numpy(np.ascontiguousarray(getattr(table, f))).to(dev)
                for f in ("dev_off", "os_class", "flags") + F64_FIELDS + BYTE_FIELDS}
        fs = _fleets_struct(table, lambda f: arrs[f].data_ptr())
        nv, nf, nd = len(variants), table.n_fleets, table.n_devices
        o = [torch.empty(nv * nf, dtype=torch.int32, device=dev), torch.empty(nv * nf, dtype=torch.float64, device=dev),
             torch.empty(nv * nd, dtype=torch.int32, device=dev), torch.empty(nv * nd, dtype=torch.int32, device=dev)]
        r = HaldaFleetResultC(*[t.data_ptr() for t in o], None, None, None, None, None)
        ms = va.model_structs(variants)

        def leg(path):
            va.set_variants_path(ctx, path)
            ts = []
            for rep in range(WARM + REPS):
                for t in o:
                    t.fill_(-7)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = lib.halda_solve_variants(ctx.ctx, ms, nv, ctypes.byref(fs), ks.ctypes.data, len(ks),
                                              ctypes.byref(r), ctypes.c_void_p(stream.cuda_stream))
                if rc != 0:
                    raise RuntimeError(f"halda_solve_variants failed ({rc}): {last_error(lib)}")
                e1.record(stream)
                stream.synchronize()
                if rep >= WARM:
                    ts.append(e0.elapsed_time(e1))
            return statistics.median(ts), va.last_variants_route(ctx), [t.cpu().numpy().tobytes() for t in o]

        rounds = {"fused": [], "loop": []}
        bits, routes = {}, {}
        for _ in range(ROUNDS):  # alternate the legs
            for leg_name, path in (("fused", 0), ("loop", 1)):
                ms_med, routes[leg_name], bits[leg_name] = leg(path)
                rounds[leg_name].append(ms_med)
        va.set_variants_path(ctx, 0)

        def timed(fn):
            for _ in range(2):
                res = fn()
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                res = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts), ts, res

        v_ms, v_all, v_res = timed(lambda: halda_solve_variants(fleets, variants))
        l_ms, l_all, l_res = timed(lambda: [halda_solve_batch(fleets, m, kv_bits=kv) for m, kv in variants])
        out[name] = {
            "workload": f"{nf} fleet(s), {nd} devices, {nv} variants, {len(ks)} k",
            "routes": routes, "same_bits": bits["fused"] == bits["loop"],
            "fused_event_ms": statistics.median(rounds["fused"]), "fused_rounds_ms": rounds["fused"],
            "loop_event_ms": statistics.median(rounds["loop"]), "loop_rounds_ms": rounds["loop"],
            "halda_solve_variants_ms": v_ms, "halda_solve_variants_all_ms": v_all,
            "python_loop_of_halda_solve_batch_ms": l_ms, "python_loop_all_ms": l_all,
            "entry_equals_loop": v_res == l_res}
    print(json.dumps(out))


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
