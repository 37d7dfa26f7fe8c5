"""Public solver API (reference: src/distilp/solver/__init__.py:5-13)."""

from .bounds import (ReplacementWithin, halda_replace_within, halda_replace_within_batch,  # noqa: F401
                     halda_solve_bounded, halda_solve_bounded_batch, move_bounds, move_box)
from .boxes import (ReloadPoint, halda_reload_frontier, halda_solve_boxes, halda_solve_boxes_batch,  # noqa: F401
                    reload_caps)
from .budget import (FrontierPoint, halda_move_frontier, halda_move_frontier_batch,  # noqa: F401
                     halda_solve_budget)
from .change import (ChangePoint, halda_change_frontier, halda_change_frontiers,  # noqa: F401
                     halda_failover_frontiers, halda_failover_plan, halda_join_frontiers)
from .coefficients import HALDAResult, ILPResult
from .fleets import halda_solve_fleets  # noqa: F401
from .halda import halda_solve, halda_solve_batch  # noqa: F401
from .plans import (PlanEvaluation, Replacement, evaluate_plan_np, halda_evaluate_plan,  # noqa: F401
                    halda_evaluate_plans_batch, halda_replace_or_keep, halda_replace_or_keep_batch)
from .scale import (ScalePoint, halda_scale_in, halda_scale_in_frontier, halda_scale_in_frontier_batch,  # noqa: F401
                    halda_scale_out_frontier)
from .subfleets import (halda_leave_one_out, halda_leave_one_out_batch, halda_select_devices,  # noqa: F401
                        halda_solve_subfleets)
from .subsets import (SubsetPoint, halda_select_devices_exact, halda_subset_frontier,  # noqa: F401
                      halda_subset_frontier_batch)
from .variants import halda_context_sweep, halda_solve_variants, model_grid  # noqa: F401

__all__ = ["halda_solve", "halda_solve_batch", "halda_solve_fleets", "halda_solve_subfleets", "halda_leave_one_out",
           "halda_leave_one_out_batch", "halda_select_devices", "halda_solve_variants", "halda_context_sweep",
           "model_grid", "halda_evaluate_plan", "halda_evaluate_plans_batch", "halda_replace_or_keep",
           "halda_replace_or_keep_batch", "halda_solve_bounded", "halda_solve_bounded_batch", "move_bounds", "move_box",
           "halda_replace_within", "halda_replace_within_batch", "ReplacementWithin", "halda_move_frontier",
           "halda_move_frontier_batch", "halda_solve_budget", "FrontierPoint", "evaluate_plan_np",
           "PlanEvaluation", "Replacement", "HALDAResult", "halda_subset_frontier", "halda_subset_frontier_batch",
           "halda_select_devices_exact", "SubsetPoint", "halda_change_frontier", "halda_change_frontiers",
           "halda_failover_frontiers", "halda_join_frontiers", "halda_failover_plan", "ChangePoint",
           "halda_scale_in_frontier", "halda_scale_in_frontier_batch", "halda_scale_in", "halda_scale_out_frontier",
           "ScalePoint", "halda_solve_boxes", "halda_solve_boxes_batch", "reload_caps", "halda_reload_frontier",
           "ReloadPoint", "ILPResult"]

__version__ = "0.1.2"  # the reference's solver module reports 0.1.2 (solver/__init__.py:13)
