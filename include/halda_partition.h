/*
 * halda_partition.h -- libhalda's entry for exact replica partitioning, beside include/halda.h (which it
 * includes: the table, model and sub-fleet types, the return codes and the ownership rules are halda.h's).
 */
#ifndef HALDA_PARTITION_H
#define HALDA_PARTITION_H

#include "halda.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * One fleet of M devices as r = 1 .. max_groups independent pipelines (halda_solve_partition).
 *
 * A group is a set of devices, written as a mask (bit i: device i). val[S] is the obj_value that
 * halda_solve_subfleets writes for the list of S's devices in ascending order, bit for bit (its k-sweep over
 * the given ks, its head rule; +inf where no k is feasible), and k[S] that entry's best_k.
 *
 * criterion 0 ("max") prices a partition by its slowest group, criterion 1 ("sum") by the sum of its groups'
 * objectives. With op(a, b) = fmax(a, b) or a + b, in this operand order:
 *     best_1[S] = val[S]
 *     best_r[S] = min over T, lowbit(S) in T, T a proper subset of S, of op(val[T], best_{r-1}[S \ T])
 * and +inf when S has fewer than r devices. The minimum is taken on the pair (value, T), lexicographic, T as
 * an unsigned integer: among equal values the smallest T wins. Under "max" that rule, not the objective,
 * decides the groups below the slowest one.
 *
 * Point r of fleet f (r = 1 .. max_groups, at f * max_groups + r - 1) is best_r of the full mask: status
 * HALDA_STATUS_OPTIMAL or _INFEASIBLE, value (+inf where infeasible), and at (f * max_groups + r - 1) * 8 + g
 * group g of the backtrack -- group 0 holds device 0, group 1 the lowest device not in group 0, and so on --
 * as its mask, its val and its k. Slots g >= r, and every slot of an infeasible point, read 0 / +inf / 0.
 * A fleet with fewer than r devices has an INFEASIBLE point r, so fleets of several sizes share one call.
 *
 * Gate, from the shapes alone, before any GPU work (HALDA_E_ARG): every fleet has 1 .. 20 devices (2^20 =
 * HALDA_SUBSETS_MAX masks); 1 <= max_groups <= 8 and max_groups <= the devices of at least one fleet;
 * criterion is 0 or 1.
 *
 * Every mask is solved on the device by the sub-fleet entry's expansion route, in launches of at most 2^21
 * listed devices; one halda_partition_level_kernel launch per level r = 2 .. max_groups follows (fleets of at
 * most 13 devices: from LDS copies of the two planes; wider ones: from the planes in global memory), then
 * halda_partition_trace_kernel. Nothing per mask leaves the device. The planes live in the context's shared
 * scratch: halda_partition_bytes(max_devices, max_groups) = 2^max_devices * (28 + 4 (max_groups - 1)) bytes
 * per fleet -- val (8 bytes a mask), k (4), two best planes (8 each), max_groups - 1 arg planes (4 each) --
 * beside the launches' item arrays; -1 outside the gate. It needs no context.
 *
 * These declarations live beside halda.h, not in it; libhalda.so exports both. HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */
typedef struct halda_partition {
    int32_t max_groups; /* R: 1 .. 8 */
    int32_t criterion;  /* 0: max, 1: sum */
} halda_partition;

typedef struct halda_partition_frontier {
    int32_t *status;      /* [n_fleets * max_groups] HALDA_STATUS_OPTIMAL / _INFEASIBLE */
    double *value;        /* [n_fleets * max_groups] */
    uint32_t *group_mask; /* [n_fleets * max_groups * 8] */
    double *group_obj;    /* [n_fleets * max_groups * 8] */
    int32_t *group_k;     /* [n_fleets * max_groups * 8] */
} halda_partition_frontier;

/* Asynchronous on `stream` (NULL = the context's stream); model, partition and ks are host memory, fleets and
 * frontier hold device arrays. With fleets of several sizes (min_devices != max_devices) it reads dev_off back
 * for the gate (it waits for `stream` once). */
int halda_solve_partition(void *ctx, const halda_model *model, const halda_fleets *fleets,
                          const halda_partition *partition, const int32_t *ks, int32_t n_k,
                          halda_partition_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe once on the way in, the points on the way out. */
int halda_solve_partition_host(void *ctx, const halda_model *model, const halda_fleets *fleets,
                               const halda_partition *partition, const int32_t *ks, int32_t n_k,
                               halda_partition_frontier *frontier);

int64_t halda_partition_bytes(int32_t max_devices, int32_t max_groups);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_PARTITION_H */
