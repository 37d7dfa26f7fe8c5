"""Sub-fleets of a packed fleet table under layer bounds (libhalda `halda_solve_subfleets_boxed`).

`halda_solve_subfleets` answers "what is the plan without this machine / with only these machines?" from one
packed table; `halda_solve_boxes_batch` keeps every device's w and n inside caps, pins and move boxes. This is
both at once: an item is (parent fleet f, index list s, box b), the fleet `[fleets[f][j] for j in s]` with list
position j bounded by box b's entry for device s[j] of fleet f. The parents are packed once, the boxes are the
planes `boxes.box_planes` writes in the parents' device layout, and the items travel as index arrays: neither
the lists nor their bounds are materialised on the host. Item i's result equals, bit for bit,
`halda_solve_bounded_batch([[fleets[f][j] for j in s]], model, [gathered bounds], route="tables")[0]`.
"""

from __future__ import annotations

import numbers
from typing import Iterable, List, Optional, Sequence

import numpy as np

from ..common import DeviceProfile, ModelProfile
from ._libhalda import last_route, set_path
from .bounds import Bounds
from .boxes import check_boxes
from .coefficients import HALDAResult
from .lower import kv_bits_to_factor
from .subfleets import _solve_arrays, pack_items


def set_subfleets_boxed_path(ctx, path: int) -> None:
    """halda_set_subfleets_boxed_path on a HaldaContext: 0 automatic (default), 1 always expand (test path)."""
    set_path(ctx, "subfleets_boxed", path)


def last_subfleets_boxed_route(ctx) -> str:
    """The route of the context's last halda_solve_subfleets_boxed call: "register", "tables", "expand", "none"."""
    return last_route(ctx, "subfleets_boxed")


def check_one_box(bounds: Sequence[Bounds], sizes: Sequence[int]) -> list:
    """One box -- `bounds` as halda_solve_bounded_batch takes it, one entry per fleet -- as check_boxes' result."""
    try:
        bounds = list(bounds)
    except TypeError:
        raise ValueError(f"bounds: {bounds!r} is not a sequence of one bounds entry per fleet") from None
    return check_boxes([bounds], sizes)


def split_items(items, n_box: int):
    """([(f, indices)], item_box int32 [n]) of items given as (f, indices) -- box 0 -- or (f, indices, b).
    ValueError for an item of another shape or a box index that is not an integer in [0, n_box)."""
    pairs, item_box = [], []
    for i, it in enumerate(items):
        try:
            n = len(it)
        except TypeError:
            n = -1
        if n not in (2, 3):
            raise ValueError(f"item {i}: {it!r} is neither (fleet, indices) nor (fleet, indices, box)")
        b = it[2] if n == 3 else 0
        if isinstance(b, bool) or not isinstance(b, numbers.Integral) or not 0 <= b < n_box:
            raise ValueError(f"item {i}: box {b!r} is not an integer in [0, {n_box})")
        pairs.append((it[0], it[1]))
        item_box.append(int(b))
    return pairs, np.asarray(item_box, np.int32)


def halda_solve_subfleets_bounded(
    fleets: Sequence[Sequence[DeviceProfile]],
    model: ModelProfile,
    items: Sequence[tuple],
    boxes: Sequence[Sequence[Bounds]],
    k_candidates: Optional[Iterable[int]] = None,
    kv_bits: str = "8bit",
    device: int = 0,
) -> List[Optional[HALDAResult]]:
    """Sub-fleets inside boxes, in one GPU call per chunk. `boxes[b]` is what halda_solve_boxes_batch takes: one
    entry per PARENT fleet, each None, (w_min, w_max) or (w_min, w_max, n_min, n_max) over that fleet's devices.
    `items[i]` is (f, indices) -- box 0 -- or (f, indices, b): indices local to fleet f, any order, repeats
    allowed. result[i] equals, bit for bit,
    halda_solve_bounded_batch([[fleets[f][j] for j in indices]], model, [bounds of those devices in box b],
    k_candidates, kv_bits, route="tables")[0]; None where the box holds no plan of the list.
    ValueError before any packing or GPU work for what halda_solve_boxes_batch refuses (an empty box list, more
    than 65,535 boxes, a box without one entry per fleet, a bad entry), a malformed item, a box index out of
    range or an empty list; IndexError for a fleet or device index out of range, as halda_solve_subfleets."""
    kv_bits_to_factor(kv_bits)
    fleets = fleets if isinstance(fleets, (list, tuple)) else list(fleets)
    sizes = np.asarray([len(d) for d in fleets], np.int64)
    checked = check_boxes(boxes, sizes.tolist())
    pairs, item_box = split_items(list(items), len(checked))
    parent, sub_off, sub_idx = pack_items(sizes, pairs)
    return _solve_arrays(fleets, model, parent, sub_off, sub_idx, k_candidates, kv_bits, device, (checked, item_box))
