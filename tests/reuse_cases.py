"""The steps a long-lived context is driven through, shared by test_reuse.py and test_gpu_reuse.py (DESIGN.md
§9, "Long-lived contexts").

A step is a Step below: the entry family, the route it must take, a shape of tests/plan_edge_cases.py with the
batch size it is run at, the fleets path set for the call, the entry ("device": halda_solve_fleets and its
kin on device arrays; "host": halda_solve_fleets_host on NumPy arrays; "python": the package's own entry on the
default context), the index of the caller's stream and the kernels last_fleet_ms must name (None where the
family has a route accessor of its own, or no launch at all). Every shape, every (case, k) and every expected
launch is plan_edge_cases's: this list invents none, so the oracle's answers are the cached ones.

Three passes over one context: SMALL in order, LARGE in reverse order, SMALL again -- the third pass runs every
kernel on buffers that held the larger call's data. Importing this module loads nothing."""

from collections import namedtuple

from . import plan_edge_cases as pe

Step = namedtuple("Step", "family route shape nf path entry stream launch")


def _s(family, route, shape, nf, path="fused", entry="device", stream=0, launch=None):
    if family == "fleets" and launch is None:
        sh = pe.shape(shape)
        launch = {"fused": sh.launch, "seg": sh.seg}[path][nf]
    return Step(family, route, shape, nf, path, entry, stream, launch)


# the smallest shape that reaches each launch
SMALL = (
    _s("fleets", "register", "m64_r64", 2),
    _s("fleets", "tables", "m64_r65", 2, stream=1),
    _s("fleets", "gated", "m2_r65", 66),
    _s("fleets", "kslot", "one_slot", 66, stream=1),
    _s("fleets", "segment", "one_slot", 66, path="seg"),
    _s("fleets", "csr", "k65", 4, stream=1),
    _s("fleets", "host_resident", "m2_r64", 1, entry="host", launch=()),   # one fleet: the resident wave, no launch
    _s("fleets", "host_zero_copy", "m64_r64", 2, entry="host"),
    _s("plan", "plan", "alone_r64", 2, launch=pe.REG),
    _s("group", "group", "alone_r64", 2, launch=pe.REG),
    _s("halda_solve", "halda_solve", "alone_r64", 2, entry="python"),  # one call per fleet
    _s("bounded", "bounded_fused", "alone_r64", 2, entry="python"),
    _s("bounded", "bounded_general", "alone_r65", 2, entry="python"),
    _s("bounded", "bounded_tables", "alone_r65", 2, entry="python"),
)

# the larger size of each family (the same shape where its case file has one size only)
LARGE = (
    _s("fleets", "register", "m64_r64", 66, stream=1),
    _s("fleets", "tables", "nf64", 64),
    _s("fleets", "gated", "m64_r65", 66, stream=1),
    _s("fleets", "kslot", "nf65", 67),
    _s("fleets", "segment", "nf65", 67, path="seg", stream=1),
    _s("fleets", "csr", "k65", 4),
    _s("fleets", "host_zero_copy", "m64_r65", 66, entry="host"),  # ~0.6 MB of dense x / c: still zero-copy
    _s("fleets", "host_copy", "nf65", 67, entry="host"),          # 1.09 MB: above kZeroCopyBytes, pinned grows
    _s("plan", "plan", "alone_r65", 2, launch=pe.TABLES),
    _s("group", "group", "alone_r65", 2, launch=pe.TABLES),
    _s("halda_solve", "halda_solve", "alone_r65", 2, entry="python"),
    _s("bounded", "bounded_general", "alone_r65", 2, entry="python"),
    _s("bounded", "bounded_tables", "alone_r65", 2, entry="python"),
)

# ---- the other families, each on the smallest and on a larger case of its own case file, through the helpers of
# its own GPU test on the default context (entry "python"). `shape` names the case (FAMILY_CASES), `nf` is the number
# of rows the call solves (instances, items, variant x fleet rows, boxes x fleets, candidates): what the family's
# grow-only buffer is sized by.
PE_FAMILIES = ("fleets", "plan", "group", "halda_solve", "bounded")


def _f(family, route, shape, nf):
    return Step(family, route, shape, nf, "fused", "python", 0, None)


FAMILY_CASES = {
    # halda_solve_batch and its settled form on host-lowered batches: pressure_cases classes (seeds 0 .. 7, kv 4bit)
    "batch16": (16,), "batch_mixed": (33, 2, 3, 5),
    # leave-one-out of two 64-device parents: plan_edge_cases shapes (one size each)
    "loo_r64": "loo_r64", "loo_r65": "loo_r65",
    # variants / plan evaluation: plan_edge_cases two-fleet shapes; variants: (shape, kv widths)
    "var2_r64": ("alone_r64", ("4bit", "8bit")), "var3_r65": ("alone_r65", ("4bit", "8bit", "fp16")),
    "var3_r64": ("alone_r64", ("4bit", "8bit", "fp16")),
    "plans_r64": "alone_r64", "plans_r65": "alone_r65",
    # boxed: box_cases (M, k, seeds); boxes: the shapes of tests/test_gpu_boxes.py (bounds_cases fleets), and
    # box_cases (M, k) against the exact oracle
    "box24": (24, 1, range(2)), "box64": (64, 1, range(3)), "box4k2": (4, 2, range(12)), "box16k2": (16, 2, range(12)),
    "reg-5x24": "reg-5x24", "reg-3x64": "reg-3x64", "tab-1x16": "tab-1x16", "tab-mixed": "tab-mixed",
    "boxes4": (4, 1), "boxes16": (16, 2),
    # budget_cases / change_cases: (list, slice); subsets_cases ENTRY_CASES index; scale_cases parent
    "budgetA": ("A", slice(0, 2)), "budgetB": ("B", slice(-2, None)),
    "changeA": ("A", slice(0, 6)), "changeB": ("B", slice(0, 24)),
    "subsets3": 0, "subsets8": 5, "subsets64": (64, 4300, 1),
    "scale4": (4, 1, 0), "scale5": (5, 2, 23),
}

FAMILY_SMALL = (
    _f("batch", "batch_and_settled", "batch16", 144),
    _f("subfleets", "subfleets_fused", "loo_r64", 128),
    _f("subfleets", "subfleets_expand", "loo_r65", 128),
    _f("variants", "variants_fused_and_loop", "var2_r64", 4),
    _f("plans", "plans_fused", "plans_r64", 2),
    _f("plans", "plans_two_launch", "plans_r64", 2),
    _f("boxed", "boxed_fused_and_general", "box24", 8),
    _f("boxed", "boxed_tables_and_general", "box4k2", 48),
    _f("boxes", "boxes_register_and_loop", "reg-5x24", 55),
    _f("boxes", "boxes_tables_and_loop", "tab-1x16", 14),
    _f("boxes", "boxes_tables", "boxes4", 18),
    _f("budget", "budget", "budgetA", 2),
    _f("change", "change", "changeA", 6),
    _f("subsets", "subsets_expand", "subsets3", 7),
    _f("change_subsets", "change_subsets", "scale4", 11),   # after halda_solve_subsets: sel_buf
    _f("subsets", "subsets_fused", "subsets64", 65),        # and before it
)
FAMILY_LARGE = (
    _f("batch", "batch_and_settled", "batch_mixed", 288),
    _f("subfleets", "subfleets_fused", "loo_r64", 128),
    _f("subfleets", "subfleets_expand", "loo_r65", 128),
    _f("variants", "variants_fused_and_loop", "var3_r64", 6),
    _f("variants", "variants_fused_and_loop", "var3_r65", 6),
    _f("plans", "plans_two_launch", "plans_r65", 2),
    _f("boxed", "boxed_fused_and_general", "box64", 12),
    _f("boxed", "boxed_tables_and_general", "box16k2", 48),
    _f("boxes", "boxes_register_and_loop", "reg-3x64", 33),
    _f("boxes", "boxes_tables_and_loop", "tab-mixed", 55),
    _f("boxes", "boxes_tables", "boxes16", 18),
    _f("budget", "budget", "budgetB", 2),
    _f("change", "change", "changeB", 24),
    _f("subsets", "subsets_expand", "subsets8", 37),
    _f("change_subsets", "change_subsets", "scale5", 16),
)
SMALL += FAMILY_SMALL
LARGE += FAMILY_LARGE

# the grow-only buffers of halda.hip and the routes whose calls size them (nf: what they are sized by)
BUFFER_ROUTES = {
    "sub_tab": ("subfleets_fused", "subfleets_expand", "subsets_expand", "subsets_fused", "change_subsets"),
    "var_desc": ("variants_fused_and_loop",),
    "sel_buf": ("subsets_expand", "subsets_fused", "change_subsets"),
    "cls": ("batch_and_settled",),
    "work": ("batch_and_settled",),
}

K_ZERO_COPY = 1 << 20  # kZeroCopyBytes of halda_solve_fleets_host


def passes():
    """The three passes of the item "every family, twice, on one context"."""
    return (("small", SMALL), ("large, reversed", LARGE[::-1]), ("small again", SMALL))


def steps():
    return [s for _, p in passes() for s in p]


def host_bytes(step):
    """A lower bound of a host step's staging size: its dense x and c alone (8 B (7 M + 1) per (fleet, k) each)."""
    sh = pe.shape(step.shape)
    return 2 * 8 * step.nf * len(sh.ks) * (7 * max(sh.sizes) + 1)


def flag_bytes(step):
    """What a step's first kernel must write of fflag: one byte per fleet."""
    return step.nf


def instances(step_list=None):
    """[(case, k)]: every distinct (case, k) with room that the steps compare, in order."""
    seen, out = set(), []
    for st in (steps() if step_list is None else step_list):
        if st.family not in PE_FAMILIES:
            continue  # held to its own case file's oracle by its own helpers
        sh = pe.shape(st.shape)
        for c in pe.batch(sh, st.nf):
            for k in pe.ks_with_room(sh, c[0]):
                if (c, k) not in seen:
                    seen.add((c, k))
                    out.append((c, k))
    return out


# ---- streams and slots: ten caller streams over the eight slots. Only a launch that uses the per-stream scratch
# takes a slot (the register launch alone takes none), and a slot is handed over least recently used first. The
# first eight streams each run a large gated batch (66 flags of 64-device fleets, 67 of 16-device ones), with
# register-only batches between them; the ninth and tenth stream, and then the first two again, take over those
# slots for smaller gated batches: stale flag bytes within the new batch's nf (66 after 66) and beyond it (66
# after 67).
N_STREAMS = 10
STREAM_STEPS = (
    _s("fleets", "gated", "m64_r65", 66, stream=0),
    _s("fleets", "kslot", "nf65", 67, stream=1),
    _s("fleets", "gated", "m64_r65", 66, stream=2),
    _s("fleets", "kslot", "nf65", 67, stream=3),
    _s("fleets", "register", "m64_r64", 2, stream=4),
    _s("fleets", "gated", "m64_r65", 66, stream=4),
    _s("fleets", "kslot", "nf65", 67, stream=5),
    _s("fleets", "register", "m64_r64", 66, stream=5),
    _s("fleets", "gated", "m64_r65", 66, stream=6),
    _s("fleets", "kslot", "nf65", 67, stream=7),
    _s("fleets", "gated", "m2_r65", 66, stream=8),    # stream 0's slot: 66 flags of the 64-device batch
    _s("fleets", "kslot", "one_slot", 66, stream=9),  # stream 1's slot: 67 flags
    _s("fleets", "register", "m64_r64", 2, stream=9),
    _s("fleets", "gated", "m1_r65", 66, stream=0),    # stream 2's slot
    _s("fleets", "kslot", "one_slot", 66, stream=1),  # stream 3's slot: 67 flags
)
SLOTS = 8

# ---- the resident wave across a pinned reallocation: (the one-fleet shape, the host call that follows it), the
# host calls growing so that each frees and reallocates the pinned buffer the wave last used
RESIDENT_ROUNDS = (
    (_s("fleets", "host_resident", "m2_r64", 1, entry="host", launch=()),
     _s("fleets", "host_zero_copy", "m64_r64", 2, entry="host")),
    (_s("fleets", "host_resident", "m64_r64", 1, entry="host", launch=()),
     _s("fleets", "host_zero_copy", "m64_r65", 66, entry="host")),
    (_s("fleets", "host_resident", "m2_r64", 1, entry="host", launch=()),
     _s("fleets", "host_copy", "nf65", 67, entry="host")),
)
