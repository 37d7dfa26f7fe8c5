/*
 * halda_subsets_boxed.h -- libhalda's entry for exact device selection under layer bounds, beside
 * include/halda.h and include/halda_subfleets_boxed.h (which it includes: the table, model, halda_subsets,
 * halda_subset_frontier and halda_boxes types, the return codes and the ownership rules are theirs).
 */
#ifndef HALDA_SUBSETS_BOXED_H
#define HALDA_SUBSETS_BOXED_H

#include "halda_subfleets_boxed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Exact device selection under boxes: "which of my machines should I use at all?", inside caps, pins,
 * disabled GPU shares and move boxes (halda_solve_subsets_boxed).
 *
 * Candidates, their enumeration order, keep_mask, the gate (fleets of 1 .. 64 devices, 0 <= max_drop <= 63 and
 * max_drop <= min(q, M - 1) of at least one fleet, no keep bit at or above M, at most HALDA_SUBSETS_MAX
 * candidates per fleet) and the tie rule (the earliest candidate among equal objectives, strict <) are
 * halda_solve_subsets', word for word.
 *
 * The boxes are n_box planes of w_min / w_max / n_min / n_max in the PARENT table's device layout -- halda_boxes
 * exactly: n_box in 1 .. 65535, box b's entry for table device g at b * nd + g with nd = dev_off[n_fleets]; any
 * of the four arrays may be NULL. A candidate's value under box b is what halda_solve_subfleets_boxed writes
 * for item (fleet, kept list, b), bit for bit: a kept device carries the box entry of its PARENT index, not of
 * its position in the kept list, and the bounds of a dropped device do not apply. A device the caller pins and
 * wants kept goes in keep_mask.
 *
 * The frontier is laid out [box][fleet][max_drop + 1]: halda_subset_frontier's four arrays, n_box times as
 * long. Point (b, f, d) is the earliest candidate of fleet f with exactly d devices dropped that has the
 * strictly lowest value under box b; it reads INFEASIBLE, +inf, mask 0, best_k 0 where the group has no
 * candidate or none feasible inside the box. With every array NULL and n_box = 1 the frontier equals
 * halda_solve_subsets' bit for bit.
 *
 * Routes, per d (halda_last_subsets_boxed_route). An item is (fleet, box, candidate); a launch takes at most
 * 2^22 items (halda_set_subsets_boxed_chunk) and is followed by halda_subsets_box_pick_kernel, one workgroup
 * per (box, fleet), which folds the launch's items into the frontier: the per-candidate values never leave
 * the device. Register route (1): every fleet of one size M and the boxed entry's fused gate over (items,
 * M - d), at most 64 k -- halda_sweep_subsets_box_kernel, one wave per item. Table route (3): else fleets of
 * any sizes whose lists' unbounded table slice fits the LDS budget, at most 64 k, fewer than 2^31 items --
 * halda_sweep_subsets_box_tables_kernel on a persistent grid. Expansion route (2; every other shape and every
 * call on path 1; the specification of the other two): halda_subsets_box_index_kernel writes items and their
 * boxes into context scratch and halda_solve_subfleets_boxed's expansion route runs on them, in chunks cut at
 * candidate boundaries. 4: the routes differ by d. The scratch is per context, so the call runs after the
 * previous user of the context's shared scratch on another stream.
 *
 * These declarations live beside halda.h, not in it: halda.h's surface is pinned as it stands; libhalda.so
 * exports both. HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */

/* Asynchronous on `stream` (NULL = the context's stream); fleets, boxes and frontier hold device arrays, model,
 * ks and keep_mask are host memory. HALDA_E_ARG (nothing launched, outputs untouched) for n_box outside
 * 1 .. 65535 and for whatever halda_solve_subsets' gate refuses. With mixed fleet sizes the call reads dev_off
 * back (it waits for `stream` once). */
int halda_solve_subsets_boxed(void *ctx, const halda_model *model, const halda_fleets *fleets,
                              const halda_subsets *subsets, const int32_t *ks, int32_t n_k, const halda_boxes *boxes,
                              halda_subset_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe once, each bound array that was passed once (all
 * n_box planes); the frontier of n_box * n_fleets * (max_drop + 1) points comes back. */
int halda_solve_subsets_boxed_host(void *ctx, const halda_model *model, const halda_fleets *fleets,
                                   const halda_subsets *subsets, const int32_t *ks, int32_t n_k,
                                   const halda_boxes *boxes, halda_subset_frontier *frontier);

/* Which routes the context's last halda_solve_subsets_boxed / _host call took: 1 the register launch for every
 * d, 3 the table launch for every d, 2 expansion for every d, 4 mixed (they differ by d), 0 when none ran yet. */
int halda_last_subsets_boxed_route(void *ctx, int *route);

/* How halda_solve_subsets_boxed runs: 0 automatic (default: a fused route where one applies), 1 always
 * expansion (test path: the fused routes are compared against it). HALDA_E_ARG for any other path. */
int halda_set_subsets_boxed_path(void *ctx, int path);

/* The most items one launch takes (0: the default, 2^22; else 1 .. 2^22). A (box, fleet, d) group cut by a
 * launch boundary is folded across the launches; a small cap exercises that fold at small shapes. The results
 * do not depend on it. HALDA_E_ARG for items < 0 or > 2^22. */
int halda_set_subsets_boxed_chunk(void *ctx, int64_t items);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_SUBSETS_BOXED_H */
