/*
 * halda_subfleets_boxed.h -- libhalda's entry for sub-fleets of a table under layer bounds, beside
 * include/halda.h and include/halda_boxes.h (which it includes: the table, model, result, halda_subfleets and
 * halda_boxes types, the return codes and the ownership rules are theirs).
 */
#ifndef HALDA_SUBFLEETS_BOXED_H
#define HALDA_SUBFLEETS_BOXED_H

#include "halda_boxes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Sub-fleets under boxes: "the plan without this machine / with only these machines", inside caps, pins and
 * move boxes (halda_solve_subfleets_boxed).
 *
 * An item is (parent fleet of `table`, list of local device indices, box index). The boxes are n_box planes of
 * w_min / w_max / n_min / n_max in the PARENT table's device layout -- halda_boxes exactly: box b's entry for
 * table device g at b * nd + g with nd = dev_off[table->n_fleets]; any of the four arrays may be NULL. Item i
 * means the fleet of its listed devices in list order (any order, repeats allowed; kappa's head by
 * halda_solve_subfleets' rule), list position j bounded by box item_box[i]'s entry for parent device idx[j].
 * item_box NULL: box 0 for every item.
 *
 * Every output of item i equals, bit for bit, what halda_solve_fleets_boxed writes for that list materialised
 * as a fleet with those bounds gathered, on a context whose bounds path is 3 (the register launch where it
 * applies, else the table launch, else the general route). Outputs are laid out as halda_solve_subfleets lays
 * them out: best_k / obj_value / obj_by_k / status / x / c / x_off per item, w / n at sub_off[i] + j. Without
 * any bound array they are halda_solve_subfleets' outputs bit for bit (bounds that never bind).
 *
 * Three routes from the shapes alone (halda_set_subfleets_boxed_path). Register route (1): every list of one
 * length M' <= 64 and the boxed entry's fused gate for (n_items, M') -- ONE launch of
 * halda_sweep_subfleets_box_kernel, one wave per item, which gathers fields and bounds from the parent table.
 * Table route (3): else lists of 1 .. 64 devices whose unbounded table slice fits the LDS budget -- ONE launch
 * of halda_sweep_subfleets_box_tables_kernel on a persistent grid. Neither uses context scratch. Expansion
 * route (2; every other shape: lists of more than 64 devices, a slice beyond the LDS budget, more than 64 k):
 * halda_expand_subfleets_kernel and halda_expand_sub_bounds_kernel write the compact table and its bounds into
 * grow-only context scratch and halda_solve_fleets_boxed runs on them under bounds path 3; the context's own
 * bounds path is put back before the call returns.
 *
 * These declarations live beside halda.h, not in it: halda.h's surface (its 71 functions and 18 structs) is
 * pinned as it stands; libhalda.so exports both. HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */
typedef struct halda_sub_boxes {
    int32_t n_box;                                 /* 1 .. 65535 */
    const int32_t *w_min, *w_max, *n_min, *n_max;  /* [n_box * dev_off[table->n_fleets]]; any may be NULL */
    const int32_t *item_box;                       /* [n_items] box of each item, NULL: box 0 */
} halda_sub_boxes;

/* Asynchronous on `stream` (NULL = the context's stream); model and ks are host memory, table, items, boxes and
 * out hold device arrays. HALDA_E_ARG (nothing launched, outputs untouched) when n_box < 1 or n_box > 65535;
 * bad item arrays or an item_box entry outside [0, n_box) are the caller's error here (not checked, as for
 * halda_solve_subfleets). On the expansion route with mixed list lengths the call reads sub_off[n_items] back
 * to size its scratch (it waits for `stream` once). */
int halda_solve_subfleets_boxed(void *ctx, const halda_model *model, const halda_fleets *table,
                                const halda_subfleets *items, const int32_t *ks, int32_t n_k,
                                const halda_sub_boxes *boxes, halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays: the parent table crosses PCIe once, each bound array that was passed
 * once, the item arrays and item_box once. Validates the items as halda_solve_subfleets_host does and every
 * item_box entry against [0, n_box): HALDA_E_ARG with a message in halda_last_error, nothing launched. */
int halda_solve_subfleets_boxed_host(void *ctx, const halda_model *model, const halda_fleets *table,
                                     const halda_subfleets *items, const int32_t *ks, int32_t n_k,
                                     const halda_sub_boxes *boxes, halda_fleet_result *out);

/* Which route the context's last halda_solve_subfleets_boxed / _host call took: 1 the register launch, 3 the
 * table launch, 2 the expansion route, 0 when none ran yet. */
int halda_last_subfleets_boxed_route(void *ctx, int *route);

/* How halda_solve_subfleets_boxed runs: 0 automatic (default: a fused route where one applies), 1 always
 * expansion (test path: the fused routes are compared against it). HALDA_E_ARG for any other path. */
int halda_set_subfleets_boxed_path(void *ctx, int path);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_SUBFLEETS_BOXED_H */
