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

/* ------------------------------------------------------------------------
 * Exact device selection and scale-in / scale-out beyond one wave (halda_solve_subsets_wide,
 * halda_solve_change_subsets_wide): fleets of up to 256 devices.
 *
 * The problems, the candidates, their enumeration order (d ascending, then ascending dropped-index lists in
 * lexicographic order), the values, the statuses and the tie rule (strict <: the earliest candidate wins) are
 * halda_solve_subsets' and halda_solve_change_subsets'; wherever both routes admit a call, status, obj, best_k,
 * loaded, released and the plans are equal bit for bit and the dropped sets are the same. What differs is how a
 * candidate is carried. There it is a 64-bit combo from a host-made list; here it is a RANK, its index in the
 * enumeration order of its (fleet, d) group, which the GPU unranks by the combinatorial number system against
 * a table of binomials C(n, j), n <= 256, j <= 63, saturated above 2^20 and built once per call. No combo list
 * is uploaded. Consequently:
 *   - keep_mask has FOUR words per fleet (bit i & 63 of word i >> 6: device i may not be dropped);
 *   - the winners are reported as dropped device INDICES, ascending, -1 padded, max_drop entries per cell
 *     (no entry at all for max_drop = 0), not as a mask;
 *   - the scale-in plans w / n have 256 entries per cell, by parent device.
 *
 * Selection: halda_rank_index_kernel (one wave per candidate) writes the chunk's candidates as
 * halda_solve_subfleets items, that entry's expansion route runs on them in chunks of at most 2^21 listed
 * devices, halda_rank_pick_kernel folds each chunk into the frontier [fleet][max_drop + 1].
 * Scale-in / scale-out: per (d, chunk) halda_change_rank_index_kernel writes the candidates with their
 * w0 / w_min / w_max, halda_solve_change_wide runs on them with max_deficit = that d's largest deficit, and
 * halda_change_rank_pick_kernel folds the chunk into the grid [fleet][d - min_drop][p]. Chunks are cut at
 * candidate boundaries so that halda_change_subsets_wide_launch_bytes stays within the context's cap (256 MiB;
 * halda_set_change_subsets_chunk), one candidate at the least.
 *
 * Gate, from the shapes (and, for scale-in, w0) alone, before any GPU work (HALDA_E_ARG; no fallback): every
 * fleet has 1 .. 256 devices; max_drop <= 63 and (selection) max_drop, (scale-in) min_drop <= min(q, M - 1) of at
 * least one fleet; no keep bit at or above M; per fleet at most HALDA_SUBSETS_MAX candidates over its d range;
 * and for scale-in every w0_i >= 0, sum w0 <= W = L / k and, per d that has a candidate, halda_solve_change_wide's
 * gate with that d's longest list and largest deficit. The scratch is per context, so the calls run after the
 * previous user of the context's shared scratch on another stream.
 * ------------------------------------------------------------------------ */
typedef struct halda_subsets_wide {
    int32_t max_drop;
    const uint64_t *keep_mask; /* HOST memory, [n_fleets * 4], or NULL */
} halda_subsets_wide;

typedef struct halda_subset_frontier_wide {
    int32_t *status;  /* [n_fleets * (max_drop + 1)] */
    double *obj;      /* the same extent */
    int32_t *dropped; /* [n_fleets * (max_drop + 1) * max_drop] */
    int32_t *best_k;  /* [n_fleets * (max_drop + 1)] */
} halda_subset_frontier_wide;

typedef struct halda_change_subsets_wide {
    const int32_t *w0;            /* [dev_off[n_fleets]] per parent device, laid out by dev_off */
    const int32_t *w_min, *w_max; /* as halda_bounds, per parent device; either may be NULL */
    int32_t min_drop, max_drop;   /* the d range */
    int32_t max_p;                /* P: the most released layers asked for, 0 .. 127 */
    const uint64_t *keep_mask;    /* HOST memory, [n_fleets * 4], or NULL */
} halda_change_subsets_wide;

typedef struct halda_change_subset_frontier_wide {
    int32_t *status;   /* [n_fleets * D1 * (max_p + 1)], D1 = max_drop - min_drop + 1 */
    double *obj;       /* the same extent */
    int32_t *dropped;  /* [n_fleets * D1 * (max_p + 1) * max_drop] */
    int32_t *loaded;   /* as status */
    int32_t *released; /* as status */
    int32_t *w, *n;    /* [n_fleets * D1 * (max_p + 1) * 256], by parent device */
} halda_change_subset_frontier_wide;

/* Asynchronous on `stream` (NULL = the context's stream); fleets and frontier hold device arrays, ks and
 * keep_mask are host memory. With mixed fleet sizes the call reads dev_off back (it waits for `stream` once). */
int halda_solve_subsets_wide(void *ctx, const halda_model *model, const halda_fleets *fleets,
                             const halda_subsets_wide *subsets, const int32_t *ks, int32_t n_k,
                             halda_subset_frontier_wide *frontier, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe on the way in, the frontier on the way back. */
int halda_solve_subsets_wide_host(void *ctx, const halda_model *model, const halda_fleets *fleets,
                                  const halda_subsets_wide *subsets, const int32_t *ks, int32_t n_k,
                                  halda_subset_frontier_wide *frontier);

/* Asynchronous on `stream` once the gate is formed: fleets, w0 / w_min / w_max and frontier hold device arrays,
 * keep_mask is host memory; the call reads dev_off and w0 back for the gate (it waits for `stream`). */
int halda_solve_change_subsets_wide(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                                    const halda_change_subsets_wide *subsets,
                                    halda_change_subset_frontier_wide *frontier, void *stream);

/* Synchronous variant on HOST arrays. */
int halda_solve_change_subsets_wide_host(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                                         const halda_change_subsets_wide *subsets,
                                         halda_change_subset_frontier_wide *frontier);

/* The bytes a launch of n_items candidates of `len` listed devices counts against the cap: the item arrays of
 * halda_change_subsets_launch_bytes and, per candidate, one workspace slice of halda_change_wide_bytes (an upper
 * bound: the launch holds one slice per resident workgroup, at most one per candidate). -1 for len < 1,
 * max_p < 0, max_deficit < 0, k < 1 or n_items < 0. No context needed. */
int64_t halda_change_subsets_wide_launch_bytes(int32_t len, int32_t max_p, int32_t max_deficit, int32_t k,
                                               int64_t n_items);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_WIDE_H */
