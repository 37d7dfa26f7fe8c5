"""`solver` CLI: load device/model profiles, run halda_solve on the GPU, print/save.

Same surface and output as the reference CLI (src/cli/solver.py:15-237):
  * --profile <folder> (falls back to test/profiles/<folder> relative to the
    working directory), or --devices ... --model ...;
  * device files sorted by name, device 0 forced to is_head=True;
  * model JSON either ModelProfileSplit (f_q has prefill/decode) -> decode-phase
    ModelProfile, or a plain ModelProfile;
  * halda_solve(devices, model, mip_gap=args.mip_gap, plot=not args.no_plot,
    kv_bits="4bit") — kv_bits is fixed to "4bit" as in the reference (:211);
    --time-limit / --max-iters / --sdisk-threshold / --k-candidates are accepted
    and ignored, as in the reference;
  * --quiet / --verbose / --save-solution formats of :176-235.
Beyond the reference: --leave-one-out prints, after the unchanged output above, one line per device with
the best k and objective of the fleet without it. --kv-sweep / --n-kv-sweep print, after that, one line per
(n_kv, kv_bits) point of the grid: the best k and objective of the fleet for that model variant.
--evaluate-solution FILE prints, last, the plan of a --save-solution JSON priced on the current fleet and its
regret / moved layers against the solution above; a file that does not name exactly the current devices is an
error (exit status 2). --max-move D (with --evaluate-solution) adds one line after those: the best plan at that
plan's k at most D layers per device away from it, `within D: k=..., obj=..., moved_layers=...`, or
`within D: infeasible`. --max-move-n Dn (with --max-move) also keeps every device's GPU share at most Dn layers
away from that plan's: the line becomes `within D (n within Dn): k=..., obj=..., moved_layers=...,
moved_gpu_layers=...`. --move-frontier B (with --evaluate-solution) prints, after those, one line per point
p = 0 .. B // 2 of the total-move-budget frontier at that plan's k (halda_move_frontier: at most p layers change
device, moved_layers <= 2 p): `frontier p: moved_layers=..., obj=..., regret=...`, or `frontier p: infeasible`.
--reload-frontier [SECONDS] (with --evaluate-solution) prints, after those, one line per point of the reload-time
frontier at that plan's k (halda_reload_frontier: the best plan reachable when every device that gains layers has
that many seconds to read them from its own disk; up to SECONDS, default every point):
`reload j: seconds=..., obj=..., regret=..., gained=[...]`, or `reload j: infeasible`.
--scale-in D (with --evaluate-solution and --failover P; --keep names devices that may not be dropped) prints, last,
one line per (d, p): `scale-in d, p: dropped=[names], loaded=..., released=..., obj=..., regret=...` or
`scale-in d, p: infeasible` (halda_scale_in_frontier's cells).
--failover P (with --evaluate-solution) prints, after those, one line per device: the best plan of the fleet
without it at that plan's k that takes at most P layers off the survivors (halda_failover_frontiers' last
point), `lose NAME: p=..., loaded=..., released=..., obj=..., regret=...`, or `lose NAME: infeasible`.
--cpu-only NAME_OR_INDEX ... solves with those devices' GPUs unused (n_max = 0 on them,
halda_solve_bounded) and prints the usual output for that solve. Without these flags the output is unchanged.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

from ..common import DeviceProfile, ModelProfile, ModelProfileSplit
from ..solver import halda_context_sweep, halda_evaluate_plan, halda_leave_one_out, halda_solve
from ..solver.plans import replacement


def load_device_profile(device_path: str) -> DeviceProfile:
    return DeviceProfile.model_validate(json.loads(Path(device_path).read_text()))


def load_model_profile(model_path: str) -> ModelProfile:
    data = json.loads(Path(model_path).read_text())
    f_q = data.get("f_q")
    if isinstance(f_q, dict) and "prefill" in f_q and "decode" in f_q:
        return ModelProfileSplit.model_validate(data).to_model_profile()
    return ModelProfile.model_validate(data)


def load_devices_and_model(device_files: List[str], model_file: str) -> Tuple[List[DeviceProfile], ModelProfile]:
    devices = [load_device_profile(f) for f in device_files]
    if devices:
        devices[0].is_head = True
    return devices, load_model_profile(model_file)


def load_from_profile_folder(profile_path: str):
    folder = Path(profile_path)
    if not folder.exists():
        folder = Path("test/profiles") / profile_path
        if not folder.exists():
            raise FileNotFoundError(f"Profile folder not found: {profile_path}")
    model_file = folder / "model_profile.json"
    if not model_file.exists():
        raise FileNotFoundError(f"model_profile.json not found in {folder}")
    device_files = sorted(str(f) for f in folder.glob("*.json") if f.name != "model_profile.json")
    if not device_files:
        raise ValueError(f"No device profiles found in {folder}")
    return load_devices_and_model(device_files, str(model_file))


def leave_one_out_lines(devices: List[DeviceProfile], model: ModelProfile, mip_gap: float) -> List[str]:
    """--leave-one-out: one line per dropped device -- its name, then the best k and obj_value of the fleet
    without it (halda_leave_one_out, kv_bits "4bit" like the solve above)."""
    res = halda_leave_one_out(devices, model, mip_gap=mip_gap, kv_bits="4bit")
    return [f"without {d.name}: " + ("infeasible" if r is None else f"k={r.k}, obj={r.obj_value:.6f}")
            for d, r in zip(devices, res)]


def variant_sweep_lines(devices: List[DeviceProfile], model: ModelProfile, mip_gap: float,
                        kv_sweep: Optional[Sequence[str]], n_kv_sweep: Optional[Sequence[int]]) -> List[str]:
    """--kv-sweep / --n-kv-sweep: one line per grid point, n_kv outermost -- n_kv, kv_bits, then the best k and
    obj_value of the fleet for that variant (halda_context_sweep). Either flag alone sweeps that axis at the
    model's other value: the model's n_kv, or the "4bit" of the solve above."""
    rows = halda_context_sweep(devices, model, n_kv_sweep or None, tuple(kv_sweep) if kv_sweep else ("4bit",),
                               mip_gap=mip_gap)
    return [f"n_kv={n}, kv_bits={kv}: " + ("infeasible" if r is None else f"k={r.k}, obj={r.obj_value:.6f}")
            for n, kv, r in rows]


class SolutionMismatch(ValueError):
    """A --evaluate-solution file that does not describe the current fleet."""


def load_incumbent(path: str, devices: List[DeviceProfile]) -> Tuple[int, List[int], List[int]]:
    """--evaluate-solution FILE: the (k, w, n) of a --save-solution JSON, matched to the current fleet by device
    name. SolutionMismatch when a name of the file is not in the fleet or a device of the fleet not in the file."""
    sol = json.loads(Path(path).read_text())
    dist = sol["layer_distribution"]
    names = [d.name for d in devices]
    extra = [n for n in dist if n not in names]
    if extra:
        raise SolutionMismatch(f"{path}: device(s) not in the current fleet: {', '.join(extra)}")
    missing = [n for n in names if n not in dist]
    if missing:
        raise SolutionMismatch(f"{path}: no entry for device(s) of the current fleet: {', '.join(missing)}")
    if int(sol["k"]) <= 0:
        raise SolutionMismatch(f"{path}: k = {sol['k']} must be positive")
    return int(sol["k"]), [int(dist[n]["w"]) for n in names], [int(dist[n]["n"]) for n in names]


def incumbent_lines(devices: List[DeviceProfile], model: ModelProfile, plan, result) -> List[str]:
    """--evaluate-solution: the incumbent priced on the current fleet (halda_evaluate_plan, kv_bits "4bit" like
    the solve above), then its regret against the solution printed above and the layers that would move."""
    k, w, _ = plan
    ev = halda_evaluate_plan(devices, model, *plan, kv_bits="4bit")
    rep = replacement(ev, plan, result)
    first = (f"incumbent: k={k}, obj={ev.obj_value:.6f}" if ev.feasible
             else f"incumbent: infeasible ({', '.join(ev.reasons)})")
    return [first, f"regret={rep.regret:.6f}, moved_layers={rep.moved_layers}"]


def within_line(devices: List[DeviceProfile], model: ModelProfile, plan, max_move: int,
                max_move_n: Optional[int] = None) -> str:
    """--max-move D: the best plan at the incumbent's k at most D layers per device away from it
    (halda_solve_bounded inside move_bounds' box), or "infeasible" when the box holds no plan. With
    --max-move-n Dn the box also keeps every n_i within Dn of the incumbent's (move_box)."""
    from ..solver.bounds import halda_solve_bounded_batch, move_bounds, move_box

    k, w, n = plan
    if max_move_n is None:
        head = f"within {max_move}"
        r = halda_solve_bounded_batch([devices], model, [move_bounds(w, max_move)], [k], kv_bits="4bit")[0]
    else:
        head = f"within {max_move} (n within {max_move_n})"
        r = halda_solve_bounded_batch([devices], model, [move_box(w, n, max_move, max_move_n)], [k],
                                      kv_bits="4bit")[0]
    if r is None:
        return f"{head}: infeasible"
    moved = sum(abs(int(a) - int(b)) for a, b in zip(r.w, w))
    line = f"{head}: k={r.k}, obj={r.obj_value:.6f}, moved_layers={moved}"
    if max_move_n is not None:
        line += f", moved_gpu_layers={sum(abs(int(a) - int(b)) for a, b in zip(r.n, n))}"
    return line


def frontier_lines(devices: List[DeviceProfile], model: ModelProfile, plan, budget: int) -> List[str]:
    """--move-frontier B: one line per point of halda_move_frontier around the incumbent (kv_bits "4bit" like
    the solve above)."""
    from ..solver.budget import halda_move_frontier

    out = []
    for p, pt in enumerate(halda_move_frontier(devices, model, plan, budget, kv_bits="4bit")):
        if pt.plan is None:
            out.append(f"frontier {p}: infeasible")
        else:
            out.append(f"frontier {p}: moved_layers={pt.moved_layers}, obj={pt.obj_value:.6f}, "
                       f"regret={pt.regret:.6f}")
    return out


def reload_lines(devices: List[DeviceProfile], model: ModelProfile, plan, max_seconds: Optional[float]) -> List[str]:
    """--reload-frontier [SECONDS]: one line per point of halda_reload_frontier around the incumbent (kv_bits
    "4bit" like the solve above)."""
    from ..solver.boxes import halda_reload_frontier

    out = []
    for j, pt in enumerate(halda_reload_frontier(devices, model, plan, max_seconds, kv_bits="4bit")):
        if pt.plan is None:
            out.append(f"reload {j}: infeasible")
        else:
            out.append(f"reload {j}: seconds={pt.seconds:.6f}, obj={pt.obj_value:.6f}, regret={pt.regret:.6f}, "
                       f"gained={pt.gained}")
    return out


def failover_lines(devices: List[DeviceProfile], model: ModelProfile, plan, max_released: int) -> List[str]:
    """--failover P: per device, the last point of its halda_failover_frontiers entry -- the best plan of the
    fleet without it that takes at most P layers off the survivors (kv_bits "4bit" like the solve above)."""
    from ..solver.change import halda_failover_frontiers

    out = []
    for dev, fr in zip(devices, halda_failover_frontiers(devices, model, plan, max_released, kv_bits="4bit")):
        pt = fr[-1]
        if pt.plan is None:
            out.append(f"lose {dev.name}: infeasible")
        else:
            out.append(f"lose {dev.name}: p={pt.released_budget}, loaded={pt.loaded}, released={pt.released}, "
                       f"obj={pt.obj_value:.6f}, regret={pt.regret:.6f}")
    return out


def pick_indices(devices: List[DeviceProfile], picks: Sequence[str]) -> List[int]:
    """NAME_OR_INDEX ...: each pick as a device index (a device's name, else its 0-based index). ValueError
    for a pick that names no device."""
    names = [d.name for d in devices]
    out = []
    for p in picks:
        if p in names:
            out.append(names.index(p))
        elif p.isdigit() and int(p) < len(devices):
            out.append(int(p))
        else:
            raise ValueError(f"{p!r} is neither a device name nor an index below {len(devices)}")
    return out


def select_lines(devices: List[DeviceProfile], model: ModelProfile, mip_gap: float, max_drop: Optional[int],
                 keep: Sequence[int]) -> List[str]:
    """--select-devices [D] [--keep ...]: one line per point of halda_subset_frontier, then the selection (the
    strict prefix-minimum over d), device names in the fleet's order (kv_bits "4bit" like the solve above)."""
    from ..solver.subsets import halda_subset_frontier, select_point

    pts = halda_subset_frontier(devices, model, max_drop, keep or None, mip_gap=mip_gap, kv_bits="4bit")
    out = []
    for d, pt in enumerate(pts):
        if pt.result is None:
            out.append(f"drop {d}: infeasible")
        else:
            out.append(f"drop {d}: dropped=[{', '.join(devices[i].name for i in pt.dropped)}], k={pt.result.k}, "
                       f"obj={pt.obj_value:.6f}")
    best = select_point(pts)
    out.append("selected: infeasible" if best is None
               else f"selected: kept=[{', '.join(devices[i].name for i in best.kept)}]")
    return out


def cpu_only_n_max(devices: List[DeviceProfile], picks: Sequence[str]) -> List[int]:
    """--cpu-only NAME_OR_INDEX ...: the n_max list with 0 on the picked devices (a device's name, else its
    0-based index in the fleet's order) and "no bound" elsewhere. ValueError for a pick that names no device."""
    names = [d.name for d in devices]
    n_max = [2**31 - 1] * len(devices)
    for p in picks:
        if p in names:
            i = names.index(p)
        elif p.lstrip("-").isdigit() and 0 <= int(p) < len(devices):
            i = int(p)
        else:
            raise ValueError(f"{p!r} is neither a device name nor an index below {len(devices)}")
        n_max[i] = 0
    return n_max


def scale_in_lines(devices: List[DeviceProfile], model: ModelProfile, plan, max_drop: int, max_released: int,
                   keep: List[int]) -> List[str]:
    """--scale-in D --failover P: one line per (d, p), d = 0 .. D devices handed back and at most p layers taken
    off the others -- the cells of halda_scale_in_frontier (kv_bits "4bit" like the solve above)."""
    from ..solver.scale import halda_scale_in_frontier

    out = []
    for d, row in enumerate(halda_scale_in_frontier(devices, model, plan, max_drop, max_released, keep=keep or None,
                                                    kv_bits="4bit")):
        for p, cell in enumerate(row):
            pt = cell.point
            if pt.plan is None:
                out.append(f"scale-in {d}, {p}: infeasible")
            else:
                names = ", ".join(devices[i].name for i in cell.dropped)
                out.append(f"scale-in {d}, {p}: dropped=[{names}], loaded={pt.loaded}, released={pt.released}, "
                           f"obj={pt.obj_value:.6f}, regret={pt.regret:.6f}")
    return out


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Run HALDA solver for distributed LLM inference optimization",
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--devices", nargs="+", help="Device profile JSON files (requires --model)")
    src.add_argument("--profile", help="Profile folder path (e.g., 'hermes_70b' or 'profiles/hermes_70b')")
    p.add_argument("--model", help="Model profile JSON file (required with --devices)")
    g = p.add_argument_group("solver parameters")
    g.add_argument("--time-limit", type=float, default=5.0, help="Time limit per k value in seconds (default: 5.0)")
    g.add_argument("--max-iters", type=int, default=50, help="Maximum outer iterations (default: 50)")
    g.add_argument("--mip-gap", type=float, default=1e-4, help="MIP gap tolerance (default: 1e-4)")
    g.add_argument("--sdisk-threshold", type=float, help="Disk speed threshold for forcing devices to M4 (bytes/s)")
    g.add_argument("--k-candidates", nargs="+", type=int, help="Specific k values to try (default: all factors of L)")
    o = p.add_argument_group("output options")
    o.add_argument("--quiet", action="store_true", help="Minimal output")
    o.add_argument("--verbose", action="store_true", help="Verbose output including device and model summaries")
    o.add_argument("--save-solution", help="Save solution to JSON file")
    o.add_argument("--no-plot", action="store_true", help="Disable plotting of k vs objective curve")
    o.add_argument("--leave-one-out", action="store_true",
                   help="After the solution, print the best k and objective of the fleet without each device")
    o.add_argument("--kv-sweep", nargs="+", metavar="BITS", choices=("4bit", "8bit", "fp16", "bf16"),
                   help="After the solution, print the best k and objective at each KV precision (e.g. 4bit 8bit fp16)")
    o.add_argument("--n-kv-sweep", nargs="+", type=int, metavar="N",
                   help="After the solution, print the best k and objective at each context length n_kv")
    o.add_argument("--evaluate-solution", metavar="FILE",
                   help="After the solution, price the plan of a --save-solution JSON on this fleet: its objective "
                        "(or why it is infeasible), its regret against the solution and the layers that would move")
    o.add_argument("--max-move", type=int, metavar="D",
                   help="With --evaluate-solution: also print the best plan at that plan's k that moves at most D "
                        "layers per device away from it")
    o.add_argument("--max-move-n", type=int, metavar="D",
                   help="With --max-move: also keep every device's GPU layers within D of that plan's")
    o.add_argument("--move-frontier", type=int, metavar="B",
                   help="With --evaluate-solution: also print, for every total budget up to B moved layers, the best "
                        "plan at that plan's k within it")
    o.add_argument("--reload-frontier", nargs="?", type=float, const=float("inf"), default=None, metavar="SECONDS",
                   help="With --evaluate-solution: also print, for every reload time up to SECONDS (default: every "
                        "point), the best plan at that plan's k whose gained layers load from disk within it")
    o.add_argument("--failover", type=int, metavar="P",
                   help="With --evaluate-solution: also print, for the loss of each device, the best plan of the "
                        "survivors at that plan's k that takes at most P layers off them")
    o.add_argument("--scale-in", type=int, metavar="D",
                   help="With --evaluate-solution and --failover P: also print, for every d up to D devices handed "
                        "back and every budget p up to P, which devices to drop and the best plan of the others")
    o.add_argument("--select-devices", nargs="?", type=int, const=-1, default=None, metavar="D",
                   help="After the solution, print the best sub-fleet with exactly d devices left out for every "
                        "d up to D (default: every subset), and the selection over them")
    o.add_argument("--keep", nargs="+", metavar="NAME_OR_INDEX", default=[],
                   help="With --select-devices or --scale-in: devices (name or 0-based index) that may not be left "
                        "out")
    g.add_argument("--cpu-only", nargs="+", metavar="NAME_OR_INDEX",
                   help="Solve without using the GPU of these devices (their name or 0-based index)")
    return p


def main(argv=None) -> int:
    parser = _parser()
    args = parser.parse_args(argv)
    bar = "=" * 60
    if args.profile:
        devices, model = load_from_profile_folder(args.profile)
        if not args.quiet:
            print(f"Loaded profile from: {args.profile}")
    elif args.devices and args.model:
        devices, model = load_devices_and_model(args.devices, args.model)
        if not args.quiet:
            print(f"Loaded {len(args.devices)} device file(s) and model")
    elif args.devices:
        parser.error("--devices requires --model")
    else:
        parser.error("Either --profile or both --devices and --model must be provided.")

    if args.max_move is not None and not args.evaluate_solution:
        parser.error("--max-move requires --evaluate-solution")
    if args.max_move is not None and args.max_move < 0:
        parser.error("--max-move must be >= 0")
    if args.max_move_n is not None and args.max_move is None:
        parser.error("--max-move-n requires --max-move")
    if args.max_move_n is not None and args.max_move_n < 0:
        parser.error("--max-move-n must be >= 0")
    if args.move_frontier is not None and not args.evaluate_solution:
        parser.error("--move-frontier requires --evaluate-solution")
    if args.move_frontier is not None and args.move_frontier < 0:
        parser.error("--move-frontier must be >= 0")
    if args.reload_frontier is not None and not args.evaluate_solution:
        parser.error("--reload-frontier requires --evaluate-solution")
    if args.reload_frontier is not None and not args.reload_frontier >= 0:
        parser.error("--reload-frontier must be >= 0")
    if args.failover is not None and not args.evaluate_solution:
        parser.error("--failover requires --evaluate-solution")
    if args.failover is not None and args.failover < 0:
        parser.error("--failover must be >= 0")
    if args.scale_in is not None and (not args.evaluate_solution or args.failover is None):
        parser.error("--scale-in requires --evaluate-solution and --failover")
    if args.scale_in is not None and args.scale_in < 0:
        parser.error("--scale-in must be >= 0")
    if args.keep and args.select_devices is None and args.scale_in is None:
        parser.error("--keep requires --select-devices or --scale-in")
    n_max = None
    if args.cpu_only:
        try:
            n_max = cpu_only_n_max(devices, args.cpu_only)
        except ValueError as e:
            print(f"error: --cpu-only: {e}", file=sys.stderr)
            return 2
    incumbent = None
    if args.evaluate_solution:
        try:
            incumbent = load_incumbent(args.evaluate_solution, devices)
        except (SolutionMismatch, OSError, KeyError, TypeError, ValueError) as e:
            print(f"error: --evaluate-solution: {e}", file=sys.stderr)
            return 2

    if args.verbose:
        print(f"\n{bar}\nLoaded {len(devices)} device(s):\n{bar}")
        for i, dev in enumerate(devices, 1):
            print(f"\n{i}. {dev.name}")
            dev.print_summary()
        model.print_summary()
    elif not args.quiet:
        print(f"\nLoaded {len(devices)} device(s) and model with {model.L} layers")

    if not args.quiet:
        print(f"\n{bar}\nRunning HALDA solver...\n{bar}")
    if n_max is None:
        result = halda_solve(devices, model, mip_gap=args.mip_gap, plot=not args.no_plot, kv_bits="4bit")
    else:
        from ..solver.bounds import halda_solve_bounded

        result = halda_solve_bounded(devices, model, n_max=n_max, kv_bits="4bit")

    if args.quiet:
        print(f"k={result.k}, obj={result.obj_value:.6f}")
        for dev, wi in zip(devices, result.w):
            print(f"{dev.name}: {wi}")
    else:
        result.print_solution(devices)

    if args.save_solution:
        payload = {
            "k": result.k,
            "objective_value": result.obj_value,
            "layer_distribution": {d.name: {"w": wi, "n": ni} for d, wi, ni in zip(devices, result.w, result.n)},
            "sets": {name: [devices[i].name for i in idx] for name, idx in result.sets.items()},
        }
        with open(args.save_solution, "w") as f:
            json.dump(payload, f, indent=2)
        if not args.quiet:
            print(f"\nSolution saved to: {args.save_solution}")
    if args.leave_one_out:
        for line in leave_one_out_lines(devices, model, args.mip_gap):
            print(line)
    if args.kv_sweep or args.n_kv_sweep:
        for line in variant_sweep_lines(devices, model, args.mip_gap, args.kv_sweep, args.n_kv_sweep):
            print(line)
    if args.select_devices is not None:
        try:
            lines = select_lines(devices, model, args.mip_gap,
                                 None if args.select_devices == -1 else args.select_devices,
                                 pick_indices(devices, args.keep))
        except (ValueError, IndexError) as e:
            print(f"error: --select-devices: {e}", file=sys.stderr)
            return 2
        for line in lines:
            print(line)
    if incumbent is not None:
        for line in incumbent_lines(devices, model, incumbent, result):
            print(line)
        if args.max_move is not None:
            if args.max_move_n is None:
                print(within_line(devices, model, incumbent, args.max_move))
            else:
                print(within_line(devices, model, incumbent, args.max_move, args.max_move_n))
        if args.move_frontier is not None:
            try:
                lines = frontier_lines(devices, model, incumbent, args.move_frontier)
            except ValueError as e:
                print(f"error: --move-frontier: {e}", file=sys.stderr)
                return 2
            for line in lines:
                print(line)
        if args.reload_frontier is not None:
            try:
                lines = reload_lines(devices, model, incumbent,
                                     None if args.reload_frontier == float("inf") else args.reload_frontier)
            except ValueError as e:
                print(f"error: --reload-frontier: {e}", file=sys.stderr)
                return 2
            for line in lines:
                print(line)
        if args.failover is not None:
            try:
                lines = failover_lines(devices, model, incumbent, args.failover)
            except ValueError as e:
                print(f"error: --failover: {e}", file=sys.stderr)
                return 2
            for line in lines:
                print(line)
        if args.scale_in is not None:
            try:
                lines = scale_in_lines(devices, model, incumbent, args.scale_in, args.failover,
                                       pick_indices(devices, args.keep))
            except (ValueError, IndexError) as e:
                print(f"error: --scale-in: {e}", file=sys.stderr)
                return 2
            for line in lines:
                print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
