"""bench.py as the driver runs it, on the GPU: a plain run prints the contract's line and, with
--dump-outputs, writes what the last timed step computed: the answers of the same seeded fleets (one
bench process per test: the run-to-run identity of the arrays follows from the fixed answers)."""

import json
import subprocess
import sys

import numpy as np
import pytest

from .conftest import REPO

pytestmark = pytest.mark.gpu

N_FLEETS, M = 96, 64


def _bench(tmp_path, name):
    out = tmp_path / name
    p = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--fleets", str(N_FLEETS), "--dump-outputs", str(out)], cwd=str(REPO), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-800:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, lines  # stdout holds the one JSON line
    return json.loads(lines[0]), {f.stem: np.load(f) for f in sorted(out.glob("*.npy"))}


def test_plain_run_dumps_the_last_steps_outputs(tmp_path, llama_online_model):
    import bench
    from distilp_amd.solver.fleets import fleet_table, solve_table

    line, got = _bench(tmp_path, "a")
    assert list(line)[:13] == ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                               "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "instances/s" and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
    inst = N_FLEETS * len(bench.KS_L80)
    assert line["config"]["instances_per_step_per_gpu"] == inst
    # value and ms_per_step state the same region (ms_per_step is printed with 6 significant digits)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / inst - 1) < 1e-5
    # a plain run carries none of the --full legs
    assert not {"roofline", "cpu_baseline", "solve_only", "c2", "batch_api", "time_to_optimal_ms"} & set(line)

    assert sorted(got) == ["best_k", "n", "obj_value", "w"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["best_k"].shape == got["obj_value"].shape == (N_FLEETS,)
    assert got["w"].shape == got["n"].shape == (N_FLEETS * M,)
    # what the library's synchronous call returns for the same seeded fleets: the integers exactly, the
    # objective to 1e-12 relative (the same FP64 formulas, -ffp-contract=off; room for nothing but order)
    want = solve_table(fleet_table(bench.build_fleets(range(N_FLEETS), M), llama_online_model), llama_online_model,
                       bench.KS_L80, 0.5)
    assert (want.best_k > 0).all()
    for k in ("best_k", "w", "n"):
        assert np.array_equal(got[k], np.asarray(getattr(want, k), np.float64).ravel()), k
    assert np.allclose(got["obj_value"], want.obj_value, rtol=1e-12, atol=0.0)
