"""The bounded sweep's table route (bounds path 3, route "tables") without a GPU: the `route` keyword's
argument check on every Python entry (before any packing or library call), the route names, and the
header's documentation of path 3."""

import pytest

from distilp_amd.solver import bounds as bd

from .conftest import REPO


@pytest.mark.parametrize("entry", ["halda_solve_bounded", "halda_solve_bounded_batch", "halda_replace_within",
                                   "halda_replace_within_batch"])
def test_a_bogus_route_is_a_value_error_before_anything_else(entry):
    """Every other argument is junk: the route is checked first, so nothing is packed and no library loaded."""
    fn = getattr(bd, entry)
    with pytest.raises(ValueError, match="route"):
        fn(None, None, None, None, route="bogus")
    with pytest.raises(ValueError, match="route"):
        fn(None, None, None, None, route=3)


def test_solve_bounded_table_checks_its_route_first():
    with pytest.raises(ValueError, match="route"):
        bd.solve_bounded_table(None, None, [1], None, None, 0.5, route="bogus")


def test_route_keyword_values():
    assert bd.check_route("auto") is None  # the context's path stays as it is
    assert bd.check_route("general") == 1 and bd.check_route("tables") == 3
    for bad in ("fused", "", None, 1, "Tables"):
        with pytest.raises(ValueError):
            bd.check_route(bad)


def test_route_names_include_tables():
    assert bd.BOUNDS_ROUTES == ("none", "fused", "general", "tables")


def test_header_documents_path_3():
    text = (REPO / "include" / "halda.h").read_text()
    doc = text[text.index("How halda_solve_fleets_bounded runs"):text.index("int halda_set_bounds_path")]
    assert "path 3" in doc and "table route" in doc
    route = text[text.index("Which route the context's last halda_solve_fleets_bounded"):
                 text.index("int halda_last_bounds_route")]
    assert "3 the table route" in route
    assert "halda_sweep_bounds_tables_kernel" in text
