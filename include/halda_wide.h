/*
 * halda_wide.h -- libhalda's second route for the total move budget and for the change frontier, beside
 * include/halda.h (which it includes: the table, model, halda_budget, halda_frontier, halda_subfleets, halda_change
 * and halda_change_frontier types, the return codes and the ownership rules are halda.h's).
 */
#ifndef HALDA_WIDE_H
#define HALDA_WIDE_H

#include "halda.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * The move frontier beyond one wave (halda_solve_fleets_budget_wide).
 *
 * The problem, the inputs and every output are halda_solve_fleets_budget's: the same halda_budget, the same
 * halda_frontier, the same statuses, tie rules and objective bits (obj is what halda_eval_plans gives the
 * returned plan), and wherever both entries admit a call their outputs are equal bit for bit. What differs is
 * the gate. halda_sweep_budget_wide_kernel runs one 256-thread workgroup per fleet: thread = device, two
 * compact value planes of (max_p + 1)^2 doubles in LDS, and the tables, the arg-min bytes and the plans in the
 * workgroup's slice of the context's global-table workspace.
 *
 * Gate, from the shapes alone: every fleet has 1 .. 256 devices, one k, 0 <= max_p <= 127, and of
 * halda_budget_wide_bytes(max_devices, max_p, k, &lds, &global) lds is at most 160 KiB and global at most
 * 2 GiB. Outside it the call returns HALDA_E_ARG and launches nothing. One launch; the workspace is per
 * context, so a launch on another stream than the workspace's previous user is ordered after it on the device.
 *
 * These declarations live beside halda.h, not in it: halda.h's surface is pinned as it stands; libhalda.so
 * exports both. HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */

/* Asynchronous on `stream` (NULL = the context's stream); fleets, budget and frontier hold device arrays. */
int halda_solve_fleets_budget_wide(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                                   const halda_budget *budget, halda_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays (frontier->n_devices is taken from dev_off); an incumbent with w0_i < 1
 * or sum w0 != L / k is HALDA_E_ARG before any GPU work, as in halda_solve_fleets_budget_host. */
int halda_solve_fleets_budget_wide_host(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                                        const halda_budget *budget, halda_frontier *frontier);

/* The two figures of the gate for this shape: *lds the workgroup's dynamic LDS, *global its workspace slice,
 * in bytes. HALDA_E_ARG for max_devices < 1, max_p < 0, k < 1 or a NULL result. No context needed. */
int halda_budget_wide_bytes(int32_t max_devices, int32_t max_p, int32_t k, int64_t *lds, int64_t *global);

/* ------------------------------------------------------------------------
 * The change frontier beyond one wave (halda_solve_change_wide).
 *
 * The problem, the inputs and every output are halda_solve_change's: the same halda_subfleets, halda_change and
 * halda_change_frontier, the same statuses (an item with some w0_i < 0, a negative deficit or one above
 * max_deficit is UNSUPPORTED), tie rules and objective bits (obj is what halda_eval_plans gives the returned
 * plan on the materialised list), and wherever both entries admit a call their outputs are equal bit for bit.
 * What differs is the gate. halda_sweep_change_wide_kernel runs one 256-thread workgroup per item: thread =
 * listed device, two value planes of (max_p + 1)(max_deficit + max_p + 1) doubles in LDS, and the tables, the
 * arg-min bytes and the plans in the workgroup's slice of the context's global-table workspace.
 *
 * Gate, from the shapes alone: every list has 1 .. 256 devices, one k, 0 <= max_p <= 127, max_deficit >= 0,
 * 2 max_p + max_deficit <= 254, and of halda_change_wide_bytes(max_devices, max_p, max_deficit, k, &lds,
 * &global) lds is at most 160 KiB and global at most 2 GiB. Outside it the call returns HALDA_E_ARG and
 * launches nothing. One launch; the workspace is per context, so a launch on another stream than the
 * workspace's previous user is ordered after it on the device.
 * ------------------------------------------------------------------------ */

/* Asynchronous on `stream` (NULL = the context's stream); table, items, change and frontier hold device arrays. */
int halda_solve_change_wide(void *ctx, const halda_model *model, const halda_fleets *table,
                            const halda_subfleets *items, int32_t k, const halda_change *change,
                            halda_change_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays, with halda_solve_change_host's checks before any GPU work (the lists, every
 * w0_i >= 0, every deficit in 0 .. max_deficit); max_deficit = -1 takes the items' largest deficit. */
int halda_solve_change_wide_host(void *ctx, const halda_model *model, const halda_fleets *table,
                                 const halda_subfleets *items, int32_t k, const halda_change *change,
                                 halda_change_frontier *frontier);

/* The two figures of the gate for this shape: *lds the workgroup's dynamic LDS, *global its workspace slice,
 * in bytes. HALDA_E_ARG for max_devices < 1, max_p < 0, max_deficit < 0, k < 1 or a NULL result. No context
 * needed. */
int halda_change_wide_bytes(int32_t max_devices, int32_t max_p, int32_t max_deficit, int32_t k, int64_t *lds,
                            int64_t *global);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_WIDE_H */
