"""Generate tests/golden/frontier_bits.npz: the move and change frontier kernels' outputs, bit for bit.

Run on the GPU against the build whose bits are to be KEPT -- before a change to the frontier kernels, the parent
commit's library (build it in a scratch worktree and point HALDA_LIB at its libhalda.so):

    HALDA_LIB=/path/to/parent/libhalda.so python tests/golden/gen_frontier_bits.py

The calls are tests/test_gpu_frontier_bits.py's CALLS; the file holds recorded results only: per call
"<call>/<output>", and "meta/items_won_by_several_T", the number of k > 1 items of budget_cases.LIST_A whose
points were won by more than one threshold T. The T that wins a point is its plan's cycle time (a plan whose
slowest device lay below T would have won at that earlier threshold with a smaller (k - 1) T), so the count is
taken from the points' plans priced by halda_eval_plans: an item counts when its OPTIMAL points, which differ in
obj, show more than one distinct cycle time.
"""

from __future__ import annotations

import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.append(str(REPO))


def main():
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime first
    from distilp_amd.common import ModelProfileSplit
    from distilp_amd.solver import _libhalda as lh
    from distilp_amd.solver import plans as pl
    from distilp_amd.solver.fleets import fleet_table
    from distilp_amd.synth import load_model_dict
    from tests import bounds_cases as bc
    from tests import budget_cases as bu
    from tests import test_gpu_frontier_bits as fb

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    out, statuses, several = {}, [], 0
    for call, run in fb.CALLS.items():
        got = run(model)
        for f, a in got.items():
            out[f"{call}/{f}"] = a
        statuses.append(got["status"].ravel())
        print(call, "status", np.bincount(got["status"].ravel(), minlength=3).tolist(), "obj", got["obj"].shape)
    for k in (2, 4):  # the thresholds that won the points of the mixed-extent budget calls at k > 1
        got = {f: out[f"budget/A34/k{k}/{f}"] for f in fb.BUDGET_FIELDS}
        fleets, _ = fb.budget_list(model, (3, 4), k)
        table = fleet_table(fleets, model)
        karr = np.full(table.n_fleets, k, np.int32)
        cyc = np.stack([pl.evaluate_table(table, model, karr, got["w"][p], got["n"][p], bc.KV).cycle.copy()
                        for p in range(max(bu.PS_A) + 1)], axis=1)
        for f in range(table.n_fleets):
            ok = got["status"][f] == lh.STATUS_OPTIMAL
            nT, nobj = len(set(cyc[f][ok].tolist())), len(set(got["obj"][f][ok].tolist()))
            several += nT > 1
            print(f"budget/A34/k{k} fleet {f}: {nobj} distinct obj, {nT} distinct T")
    st = np.concatenate(statuses)
    assert (st == lh.STATUS_OPTIMAL).any() and (st == lh.STATUS_INFEASIBLE).any()
    assert several >= 1, several
    out["meta/items_won_by_several_T"] = np.asarray(several, np.int64)
    np.savez_compressed(fb.GOLDEN, **out)
    size = fb.GOLDEN.stat().st_size
    print(f"{lh.LIB_PATH}: {len(fb.CALLS)} calls, {several} items won by several T, {size} bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
