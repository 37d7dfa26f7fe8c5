"""Route "wide" of device selection and scale-in / scale-out without a GPU: the host mirror of the GPU's
unranking against itertools' order, and the gates."""

import itertools
import math

import pytest

from distilp_amd.solver import scale as sc
from distilp_amd.solver import subsets as ss

from . import bounds_cases as bc
from . import deep_cases as dc


@pytest.mark.parametrize("q,d", [(5, 2), (65, 1), (66, 2), (130, 2), (20, 10)])
def test_unrank_is_itertools_order(q, d):
    n = math.comb(q, d)
    ranks = set(range(n)) if n <= 10000 else {0, 1, n // 3, n // 2, n - 2, n - 1}
    seen = 0
    for r, c in enumerate(itertools.combinations(range(q), d)):
        if r in ranks:
            assert ss.unrank(q, d, r) == list(c), (q, d, r)
            seen += 1
    assert seen == len(ranks)
    assert ss.binom_table()[d][q] == min(n, ss.RANK_SAT)


@pytest.mark.parametrize("M,max_drop,keep,route", [(257, 1, None, "wide"), (256, 3, None, "wide"), (65, 1, [65], "wide"),
                                                   (65, 1, None, "tables")])
def test_wide_gates_raise_before_any_gpu_work(llama_online_model, M, max_drop, keep, route):
    """257 devices; more than 2^20 candidates; a keep index at M; an unknown route."""
    model = dc.model_at(llama_online_model, 512)
    devs = (list(bc.devices(64, 0)) * 5)[:M]
    with pytest.raises(ValueError):
        ss.halda_subset_frontier(devs, model, max_drop, keep, kv_bits="4bit", route=route)
    with pytest.raises(ValueError):
        sc.halda_scale_in_frontier(devs, model, (1, [1] * (M - 1) + [513 - M], [0] * M), max_drop, 1, keep=keep,
                                   kv_bits="4bit", route=route)


def test_wave_route_on_65_devices_raises_what_it_raises_today(llama_online_model):
    model, devs = llama_online_model, list(bc.devices(64, 0)) + [bc.devices(64, 0)[0]]
    inc = (1, [1] * 64 + [int(model.L) - 64], [0] * 65)
    for kw in ({}, {"route": "wave"}):
        with pytest.raises(ValueError, match="exact selection needs fleets of at most 64 devices, fleet 0 has 65"):
            ss.halda_subset_frontier(devs, model, 1, **kw)
        with pytest.raises(ValueError, match="scale-in needs fleets of at most 64 devices, fleet 0 has 65"):
            sc.halda_scale_in_frontier(devs, model, inc, 1, 1, **kw)
        with pytest.raises(ValueError, match="scale-out needs at most 64 devices in fleet and pool, got 65"):
            sc.halda_scale_out_frontier(devs[:64], devs[64:], model, (1, [1] * 63 + [17], [0] * 64), 1, 1, **kw)
