/*
 * halda_boxes_wide.h -- libhalda's workgroup entry for one fleet table under many boxes, beside
 * include/halda_boxes.h (which it includes: halda_boxes, and through it halda.h's table, model and result types,
 * return codes and ownership rules).
 */
#ifndef HALDA_BOXES_WIDE_H
#define HALDA_BOXES_WIDE_H

#include "halda_boxes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Many boxes beyond one wave (halda_solve_fleets_boxes_wide).
 *
 * halda_solve_fleets_boxes' problem, inputs and box-major outputs (best_k, obj_value, w, n and the optional
 * obj_by_k / status) in ONE launch of halda_sweep_boxes_wide_kernel: one 256-thread workgroup per (box, fleet),
 * which builds the fleet's bounded tables from the device fields and solves every k of `ks` by a dynamic
 * programme over the layers handed out above sum wlo (k > 1: a pass per threshold candidate). x / c are not
 * produced: out->x, out->c and out->x_off must be NULL. The objective of an OPTIMAL (box, fleet, k) is
 * halda_eval_plans' device-formed objective of the returned (k, w, n), bit for bit; statuses follow
 * halda_solve_fleets_boxed's ladder. Ties: the least w_i within a transition, the earliest threshold, the
 * smallest k.
 *
 * The gate is formed from the shapes alone; outside it HALDA_E_ARG and nothing launched: fleets of 1 .. 256
 * devices (any mix), 1 <= n_box <= 65535, n_k <= 64, n_box * n_fleets * n_k < 2^31, and with
 * max_R = max(0, L / ks[0] - min_devices) the LDS bytes of halda_boxes_wide_bytes within 160 KiB and its
 * workspace bytes (one workgroup's slice of the context's global tables) within 2 GiB.
 *
 * These declarations live beside halda_boxes.h, not in it: that header's surface is pinned as it stands;
 * libhalda.so exports both. HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */

/* Asynchronous on `stream` (NULL = the context's stream); model and ks are host memory, fleets, boxes and out
 * hold device arrays. */
int halda_solve_fleets_boxes_wide(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                                  int32_t n_k, const halda_boxes *boxes, halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe once on the way in, each bound array that was passed
 * once, the n_box result slices on the way out. */
int halda_solve_fleets_boxes_wide_host(void *ctx, const halda_model *model, const halda_fleets *fleets,
                                       const int32_t *ks, int32_t n_k, const halda_boxes *boxes,
                                       halda_fleet_result *out);

/* The LDS bytes of one workgroup and the bytes of its workspace slice for fleets of up to max_devices devices and
 * rows of up to max_R + 1 entries; any_k_gt_1 != 0 when some k of the call is > 1 (the H table and its row
 * buffers). HALDA_E_ARG for max_devices < 1, max_R < 0 or a NULL result. */
int halda_boxes_wide_bytes(int32_t max_devices, int32_t max_R, int32_t any_k_gt_1, int64_t *lds, int64_t *global);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_BOXES_WIDE_H */
