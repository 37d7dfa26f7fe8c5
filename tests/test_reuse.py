"""The step list of tests/reuse_cases.py is what test_gpu_reuse.py needs it to be ("Long-lived
contexts"): every shape, (case, k) and expected launch is plan_edge_cases's, every family and route is reached,
the passes hold the larger-then-smaller pairs and the stream list the slot take-overs, and the instances the
steps compare are held to the oracle's uniqueness and slack floors. No GPU, no libhalda."""

import pytest

from . import plan_edge_cases as pe
from . import reuse_cases as rc

ALL_STEPS = (rc.steps() + list(rc.STREAM_STEPS) + [s for pair in rc.RESIDENT_ROUNDS for s in pair])

# what the passes must reach: family -> routes (a route named "a_and_b" runs both in one step)
WANT = {
    "fleets": {"register", "tables", "gated", "kslot", "segment", "csr", "host_resident", "host_zero_copy",
               "host_copy"},
    "plan": {"plan"}, "group": {"group"}, "halda_solve": {"halda_solve"},
    "bounded": {"bounded_fused", "bounded_general", "bounded_tables"},
    "batch": {"batch_and_settled"},
    "subfleets": {"subfleets_fused", "subfleets_expand"},
    "variants": {"variants_fused_and_loop"},
    "plans": {"plans_fused", "plans_two_launch"},
    "boxed": {"boxed_fused_and_general", "boxed_tables_and_general"},
    "boxes": {"boxes_register_and_loop", "boxes_tables_and_loop", "boxes_tables"},
    "budget": {"budget"}, "change": {"change"},
    "subsets": {"subsets_fused", "subsets_expand"},
    "change_subsets": {"change_subsets"},
}
ROUTE_LAUNCH = {"register": pe.REG, "tables": pe.TABLES, "gated": pe.REG_GATED, "kslot": pe.KSLOT,
                "segment": pe.SEG, "csr": pe.CSR}


def test_every_step_is_a_shape_and_a_case_of_the_plan_edge_list():
    names = {sh.name for sh in pe.STATIC_SHAPES}
    listed = set(pe.instances(pe.STATIC_SHAPES))
    for st in ALL_STEPS:
        if st.family not in rc.PE_FAMILIES:
            continue
        assert st.shape in names, st
        sh = pe.shape(st.shape)
        assert 1 <= st.nf and st.path in ("fused", "seg") and st.entry in ("device", "host", "python"), st
        for c in pe.batch(sh, st.nf):
            assert c in pe.cases_of(sh), (st, c)
            for k in pe.ks_with_room(sh, c[0]):
                assert (c, k) in listed, (st, c, k)
    assert set(rc.instances(ALL_STEPS)) <= listed


def test_expected_kernels_are_the_plan_edge_lists():
    """A fleets step's kernels are what plan_edge_cases gives its shape at its batch size on its path; the host
    steps have the device entry's launch, and a one-fleet host step on a register-only shape has none (the
    resident wave answers it)."""
    for st in ALL_STEPS:
        if st.family != "fleets":
            continue
        sh = pe.shape(st.shape)
        if st.route == "host_resident":
            assert st.nf == 1 and st.entry == "host" and st.launch == (), st
            assert set(sh.launch.values()) == {pe.REG}, st  # register-only at every batch size
            continue
        by_path = sh.launch if st.path == "fused" else sh.seg
        assert st.launch == by_path[st.nf], st
        if st.route in ROUTE_LAUNCH:
            assert st.launch == ROUTE_LAUNCH[st.route], st
    for st in rc.steps():
        if st.family in ("plan", "group"):
            assert st.launch == pe.shape(st.shape).launch[st.nf], st


def test_the_passes_reach_every_family_and_route():
    everything = {(f, r) for f, rs in WANT.items() for r in rs}
    # the small pass has no call above the zero-copy size; the large one no one-fleet call and no fused bounded
    # sweep (R + 1 = 64 is that route's only size)
    absent = {"small": {("fleets", "host_copy")},
              "large": {("fleets", "host_resident"), ("bounded", "bounded_fused"), ("plans", "plans_fused"),
                        ("subsets", "subsets_fused")}}  # (the fused plan and subset routes have one size each)
    for name, steps in rc.passes():
        got = {(st.family, st.route) for st in steps}
        assert got == everything - absent[name.split(",")[0].split()[0]], (name, everything - got)
    reached = {(st.family, st.route) for st in rc.steps()}
    assert reached == {(f, r) for f, rs in WANT.items() for r in rs}
    assert {st.entry for st in rc.steps()} == {"device", "host", "python"}
    assert len({st.stream for st in rc.steps() if st.entry == "device"}) > 1


def _pairs(steps, pred, size):
    """Whether some step with `pred` is followed, later in `steps`, by one with a smaller `size`."""
    sel = [size(s) for s in steps if pred(s)]
    return any(a > b for i, a in enumerate(sel) for b in sel[i + 1:])


def test_larger_then_smaller_pairs_for_the_grow_only_buffers():
    """scratch and pinned (a host step's staging bytes), the zero-copy threshold crossed downwards, fflag (a
    gated step's flag bytes -- and, at equal counts, a 66-flag batch of other fleets before it), the table
    kernel's LDS (layers x devices) and the fleet scratch (total devices x k of a device step)."""
    steps = [s for s in rc.steps() if s.family in rc.PE_FAMILIES]
    host = lambda s: s.entry == "host"  # noqa: E731
    assert _pairs(steps, host, rc.host_bytes)
    sizes = [rc.host_bytes(s) for s in steps if host(s)]
    over = [i for i, b in enumerate(sizes) if b > rc.K_ZERO_COPY]
    assert over and any(b <= rc.K_ZERO_COPY for b in sizes[over[0] + 1:]), sizes  # copy route, then zero-copy again
    assert min(sizes) < 4096  # a single fleet's few hundred bytes after 1 MiB
    gated = lambda s: s.entry == "device" and s.route in ("gated", "kslot", "segment")  # noqa: E731
    assert _pairs(steps, gated, rc.flag_bytes)
    assert _pairs(steps, lambda s: s.family == "fleets" and s.entry == "device",
                  lambda s: s.nf * max(pe.shape(s.shape).sizes) * len(pe.shape(s.shape).ks))
    assert _pairs(steps, lambda s: s.route == "tables", lambda s: pe.shape(s.shape).L * max(pe.shape(s.shape).sizes))
    # a resident-wave call after the pinned buffer grew past it, three times with growing sizes
    big = [rc.host_bytes(b) for _, b in rc.RESIDENT_ROUNDS]
    assert len(big) == 3 and big == sorted(set(big)) and big[-1] > rc.K_ZERO_COPY > big[0]
    assert all(one.route == "host_resident" for one, _ in rc.RESIDENT_ROUNDS)


def test_the_stream_list_takes_slots_over_for_smaller_gated_batches():
    """Replays the slot rule (a stream keeps its slot; a new stream takes a free slot, else the least recently
    used) over STREAM_STEPS: more streams than slots, and a take-over by a gated batch with fewer flags than the
    slot last held as well as one with as many."""
    slots, tick = {}, 0   # stream -> [tick, flags last written]
    fewer = equal = 0
    for st in rc.STREAM_STEPS:
        if st.launch == pe.REG:
            continue  # the register launch alone takes no slot
        tick += 1
        if st.stream not in slots:
            held = None
            if len(slots) == rc.SLOTS:
                lru = min(slots, key=lambda s: slots[s][0])
                held = slots.pop(lru)[1]
            if held is not None and st.launch != pe.TABLES:
                fewer += rc.flag_bytes(st) < held
                equal += rc.flag_bytes(st) == held
        slots[st.stream] = [tick, rc.flag_bytes(st)]
    assert len({st.stream for st in rc.STREAM_STEPS}) == rc.N_STREAMS > rc.SLOTS
    assert fewer >= 1 and equal >= 1, (fewer, equal)
    assert any(st.launch == pe.REG for st in rc.STREAM_STEPS)


@pytest.mark.parametrize("which", ["passes", "all"])
def test_compared_instances_are_unique_and_use_slack(which):
    """At least 95 % of the feasible instances the steps compare have a unique optimum by the oracle's margin, and
    every family compares at least one instance with a positive slack or t column. Conditions on the case
    choice: a case that misses them is replaced, not the floor."""
    steps = rc.steps() if which == "passes" else ALL_STEPS
    sh = pe.shares(rc.instances(steps))
    print(f"{which}: {len(steps)} steps, {sh}")
    assert sh["feasible"] > 0 and sh["unique"] >= 0.95 * sh["feasible"], sh
    for fam in rc.PE_FAMILIES:  # (the other families are held to their own case files' recorded oracles)
        inst = rc.instances([s for s in steps if s.family == fam])
        assert any(pe.has_slack_or_t(c, k) for c, k in inst), fam


def test_the_other_families_cases_are_in_their_own_case_files():
    """A step outside the plan-edge families names a case of its family's own list: nothing is invented."""
    from . import budget_cases as bu
    from . import change_cases as cc
    from . import pressure_cases as pc
    from . import scale_cases as sx
    from . import subsets_cases as sc

    C = rc.FAMILY_CASES
    for st in rc.FAMILY_SMALL + rc.FAMILY_LARGE:
        assert st.shape in C and st.entry == "python", st
    for name in ("batch16", "batch_mixed"):
        assert all(pc.cases(Ms=(M,), kvs=("4bit",), seeds=range(8)) for M in C[name])
    shapes = {sh.name for sh in pe.STATIC_SHAPES}
    assert {C["loo_r64"], C["loo_r65"], C["plans_r64"], C["plans_r65"]} <= shapes
    assert all(C[n][0] in shapes for n in ("var2_r64", "var3_r64", "var3_r65"))
    for name, lists in (("budgetA", bu.LIST_A), ("budgetB", bu.LIST_B)):
        assert len(lists[C[name][1]]) == 2
    assert len({(M, k, s) for M, k, s in cc.LIST_A + cc.LIST_B}) == len(cc.LIST_A + cc.LIST_B)
    assert C["subsets3"] < len(sc.ENTRY_CASES) and sc.ENTRY_CASES[C["subsets8"]][1] == 8
    assert C["scale4"] in sx.PARENTS and C["scale5"] in sx.EXTRA


def test_subsets_and_change_subsets_are_adjacent_in_both_orders():
    """halda_solve_subsets and halda_solve_change_subsets share sel_buf: some pass runs one right after the
    other, and some pass the other way round."""
    orders = set()
    for _, steps in rc.passes():
        for a, b in zip(steps, steps[1:]):
            if {a.family, b.family} == {"subsets", "change_subsets"}:
                orders.add((a.family, b.family))
    assert orders == {("subsets", "change_subsets"), ("change_subsets", "subsets")}, orders


def test_larger_then_smaller_pairs_for_the_families_buffers():
    """sub_tab, var_desc, sel_buf, cls and work: over the three passes some call of a route that sizes the buffer
    is followed by one with fewer rows. (gtab has no pair: it is sized by the global-table launch, which one shape
    of the lists reaches -- lds_over, whose L comes from libhalda -- at one batch size.)"""
    steps = rc.steps()
    for buf, routes in rc.BUFFER_ROUTES.items():
        assert _pairs(steps, lambda s: s.route in routes, lambda s: s.nf), buf
