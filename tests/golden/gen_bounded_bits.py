"""Generate tests/golden/bounded_bits.npz: the bounded sweep's outputs under binding bounds, bit for bit.

Run on the GPU against the build whose bits are to be KEPT -- before a change to the bounded kernels, the parent
commit's library (build it in a scratch worktree and point HALDA_LIB at its libhalda.so):

    HALDA_LIB=/path/to/parent/libhalda.so python tests/golden/gen_bounded_bits.py

The calls are tests/test_gpu_bounded_bits.py's (CALLS, replayed by its replay()); the file holds recorded results
only: per call "<shape>/<variant>/<output>" for the outputs recorded(shape) names, and ".../route".
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
    from distilp_amd.synth import load_model_dict
    from tests import test_gpu_bounded_bits as bb

    model = ModelProfileSplit.model_validate(load_model_dict()).to_model_profile()
    ctx = lh.get_context(0)
    out = {}
    for shape, variant in bb.CALLS:
        got, route = bb.replay(ctx, model, shape, variant)
        assert route == bb.SHAPES[shape][0], (shape, variant, route)
        out[f"{shape}/{variant}/route"] = np.asarray(route)
        for f in bb.recorded(shape):
            out[f"{shape}/{variant}/{f}"] = got[f]
        print(shape, variant, route, "status", np.bincount(got["status"]).tolist(), "best_k", got["best_k"].tolist())
    np.savez_compressed(bb.GOLDEN, **out)
    size = bb.GOLDEN.stat().st_size
    print(f"{lh.LIB_PATH}: {len(bb.CALLS)} calls, {size} bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
