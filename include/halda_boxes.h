/*
 * halda_boxes.h -- libhalda's entry for one fleet table under many boxes, beside include/halda.h (which it
 * includes: the table, model, result and halda_box types, the return codes and the ownership rules are
 * halda.h's).
 */
#ifndef HALDA_BOXES_H
#define HALDA_BOXES_H

#include "halda.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * One table under many boxes: a ladder of caps, a set of what-ifs (halda_solve_fleets_boxes).
 *
 * halda_boxes holds n_box boxes on the one table: each of the four arrays, where passed, holds n_box planes
 * of nd = dev_off[n_fleets] entries, box-major (box b's entry for table device i at b * nd + i), with the
 * meaning and the "no bound" values of halda_box. Outputs are box-major, halda_solve_variants' layout with
 * "variant" read as "box": with nf = n_fleets, best_k / obj_value hold n_box * nf entries (box b, fleet f at
 * b * nf + f), w / n hold n_box * nd (box b's block at b * nd), obj_by_k / status n_box * nf * n_k, x / c are
 * dense with stride 7 max_devices + 1 over (b, f, k), or compact through an x_off of n_box * nf * n_k entries
 * (element offsets into the one x / c, -1: not wanted). Slice b of every output equals, bit for bit, what
 * halda_solve_fleets_boxed writes for box b alone (the four arrays' planes b, an array that is NULL here NULL
 * there) on a context whose bounds path is 3: the register launch where it applies, else the table launch,
 * else the general route.
 *
 * Three routes, one contract (halda_set_boxes_path), gated as the boxed entry gates them. Register route:
 * under its fused gate ONE launch of halda_sweep_boxes_kernel, one wave per (box, fleet). Table route: else,
 * under path 3's table gate, ONE launch of halda_sweep_boxes_tables_kernel over the n_box * nf items on the
 * table kernel's LDS slice (the slice depends on the unbounded shape only, so one serves every box). Neither
 * uses context scratch; with an n array the waves run on box records, without one on bound records, as the
 * boxed entry chooses its kernel. Loop route (every other shape: fleets of more than 64 devices, a slice
 * beyond the LDS budget, more than 64 k, n_box * nf * n_k >= 2^31, the CSR pipeline): n_box
 * halda_solve_fleets_boxed calls on the caller's stream under bounds path 3 with the pointers moved.
 * The call does not change the context's bounds path as halda_set_bounds_path left it; on the loop route
 * halda_last_bounds_route afterwards reports the last box's route, on the other two it is left alone.
 *
 * These declarations live beside halda.h, not in it: halda.h's surface (its 71 functions and 18 structs) is
 * pinned as it stands; libhalda.so exports both. HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */
typedef struct halda_boxes {
    int32_t n_box;                                 /* 1 .. 65535 */
    const int32_t *w_min, *w_max, *n_min, *n_max;  /* [n_box * dev_off[n_fleets]]; any may be NULL (= no bound) */
} halda_boxes;

/* Asynchronous on `stream` (NULL = the context's stream); model and ks are host memory, fleets, boxes and out
 * hold device arrays. HALDA_E_ARG (nothing launched) when n_box < 1 or n_box > 65535. On the loop route a call
 * with n_box > 1 reads dev_off[n_fleets] back to place the slices (it waits for `stream` once). */
int halda_solve_fleets_boxes(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_boxes *boxes, halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays (x_off host memory too): the table crosses PCIe once on the way in, each
 * bound array that was passed once, the n_box result slices on the way out. It knows dev_off[n_fleets], so it
 * never reads it back. */
int halda_solve_fleets_boxes_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                                  int32_t n_k, const halda_boxes *boxes, halda_fleet_result *out);

/* Which route the context's last halda_solve_fleets_boxes / _host call took: 1 the register launch, 3 the
 * table launch, 2 the per-box loop, 0 when none ran yet. */
int halda_last_boxes_route(void *ctx, int *route);

/* How halda_solve_fleets_boxes runs: 0 automatic (default: a fused route where one applies), 1 always loop
 * (test path: the fused routes are compared against it). HALDA_E_ARG for any other path. */
int halda_set_boxes_path(void *ctx, int path);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_BOXES_H */
