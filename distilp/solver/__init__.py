"""Alias of distilp_amd.solver (reference API: distilp.solver.halda_solve / HALDAResult)."""

from distilp_amd.solver import HALDAResult, ILPResult, halda_solve, halda_solve_batch  # noqa: F401
from distilp_amd.solver import (halda_leave_one_out, halda_leave_one_out_batch, halda_select_devices,  # noqa: F401
                                halda_solve_subfleets)
from distilp_amd.solver import halda_context_sweep, halda_solve_variants, model_grid  # noqa: F401
from distilp_amd.solver import (PlanEvaluation, Replacement, evaluate_plan_np, halda_evaluate_plan,  # noqa: F401
                                halda_evaluate_plans_batch, halda_replace_or_keep, halda_replace_or_keep_batch)
from distilp_amd.solver import (ReplacementWithin, halda_replace_within, halda_replace_within_batch,  # noqa: F401
                                halda_solve_bounded, halda_solve_bounded_batch, move_bounds, move_box)
from distilp_amd.solver import (FrontierPoint, halda_move_frontier, halda_move_frontier_batch,  # noqa: F401
                                halda_solve_budget)
from distilp_amd.solver import (SubsetPoint, halda_select_devices_exact, halda_subset_frontier,  # noqa: F401
                                halda_subset_frontier_batch)
from distilp_amd.solver import (ChangePoint, halda_change_frontier, halda_change_frontiers,  # noqa: F401
                                halda_failover_frontiers, halda_failover_plan, halda_join_frontiers)
from distilp_amd.solver import (ScalePoint, halda_scale_in, halda_scale_in_frontier,  # noqa: F401
                                halda_scale_in_frontier_batch, halda_scale_out_frontier)
from distilp_amd.solver import (ReloadPoint, halda_reload_frontier, halda_solve_boxes,  # noqa: F401
                                halda_solve_boxes_batch, reload_caps)

__all__ = ["halda_solve", "HALDAResult"]

__version__ = "0.1.2"
