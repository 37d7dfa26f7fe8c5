/*
 * halda_partition_classes.h -- exact replica partitioning by device class, beside include/halda_partition.h
 * (which it includes: the criteria, the recurrence's operand order and the point layout are that header's).
 */
#ifndef HALDA_PARTITION_CLASSES_H
#define HALDA_PARTITION_CLASSES_H

#include "halda_partition.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * One fleet of up to 256 devices of a few kinds as r = 1 .. max_groups pipelines
 * (halda_solve_partition_classes).
 *
 * Classes. The devices of one fleet whose table rows are equal in every field of halda_fleets (flags
 * included) form a class. Classes are numbered by first occurrence; cnt_c is the size of class c. The fleet's
 * class order lists its devices class-major, ascending index within a class. The entry takes the class id of
 * every device from the caller and trusts that equal ids mean equal rows.
 *
 * Groups. A group is a count vector g, 0 <= g_c <= cnt_c, not all zero. Its code is sum g_c * stride_c with
 * stride_0 = 1 and stride_{c+1} = stride_c * (cnt_c + 1), so code(S - T) = code(S) - code(T) with no borrow
 * wherever T <= S componentwise. val[g] and k[g] are what halda_solve_subfleets writes for the list "the first
 * g_c devices of every class, in class order", bit for bit. That list is class-major, not ascending by index:
 * the sub-fleet entry takes any order, and its head rule (first listed HALDA_DEV_HEAD device, else the first
 * listed) then depends on the counts alone -- devices of one class are interchangeable, so every set of
 * devices with these counts has this value.
 *
 * Recurrence, with the criteria and op of halda_partition.h:
 *     best_1[S] = val[S]
 *     best_r[S] = min over T of op(val[T], best_{r-1}[S - T])
 * over 0 <= T <= S componentwise with T != S and T_c0 >= 1, c0 the lowest class present in S (the mask route's
 * "T holds the lowest device of S"); +inf when S has fewer than r devices. The minimum is taken on the pair
 * (value, code(T)), lexicographic: among equal values the smallest code wins.
 *
 * Point r of fleet f (at f * max_groups + r - 1) is best_r of the full count vector: status, value, and at
 * (f * max_groups + r - 1) * 8 + g group g of the backtrack as its code, its val and its k. Slots g >= r, and
 * every slot of an infeasible point, read 0 / +inf / 0.
 *
 * Gate, from the shapes alone, before any GPU work (HALDA_E_ARG): every fleet has 1 .. 256 devices in at most
 * 8 classes (ids 0 .. 7, numbered by first occurrence), at most 2^20 codes prod (cnt_c + 1), and at most 2^32
 * pair evaluations a level, prod (cnt_c + 1)(cnt_c + 2) / 2; 1 <= max_groups <= 8 and max_groups <= the
 * devices of at least one fleet; criterion is 0 or 1.
 *
 * Every code is solved on the device by the sub-fleet entry's expansion route, in launches of at most 2^21
 * listed devices (halda_partition_classes_index_kernel writes the lists); one
 * halda_partition_classes_level_kernel launch per level r = 2 .. max_groups follows (every fleet of at most
 * 8192 codes: from LDS copies of the two planes; otherwise from the planes in global memory), then
 * halda_partition_classes_trace_kernel. Nothing per code leaves the device. The planes are the mask route's,
 * per code, in the context's shared scratch: halda_partition_classes_bytes(counts, n_classes, max_groups) =
 * prod (counts[c] + 1) * (28 + 4 (max_groups - 1)) bytes per fleet, -1 outside the gate. It needs no context.
 *
 * libhalda.so exports these beside halda.h's; HALDA_ABI_VERSION stays 3.
 * ------------------------------------------------------------------------ */
typedef struct halda_partition_classes {
    int32_t max_groups;     /* R: 1 .. 8 */
    int32_t criterion;      /* 0: max, 1: sum */
    const int32_t *cls;     /* HOST [dev_off[n_fleets]] class id of every device, within its fleet */
    const int64_t *dev_off; /* HOST [n_fleets + 1] the table's dev_off */
} halda_partition_classes;

typedef struct halda_partition_classes_frontier {
    int32_t *status;      /* [n_fleets * max_groups] HALDA_STATUS_OPTIMAL / _INFEASIBLE */
    double *value;        /* [n_fleets * max_groups] */
    uint32_t *group_code; /* [n_fleets * max_groups * 8] */
    double *group_obj;    /* [n_fleets * max_groups * 8] */
    int32_t *group_k;     /* [n_fleets * max_groups * 8] */
} halda_partition_classes_frontier;

/* Asynchronous on `stream` (NULL = the context's stream); model, classes (and the arrays it points to) and ks
 * are host memory, fleets and frontier hold device arrays. It reads nothing back. */
int halda_solve_partition_classes(void *ctx, const halda_model *model, const halda_fleets *fleets,
                                  const halda_partition_classes *classes, const int32_t *ks, int32_t n_k,
                                  halda_partition_classes_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe once on the way in, the points on the way out.
 * classes->dev_off may be NULL: the table's own dev_off is host memory here. */
int halda_solve_partition_classes_host(void *ctx, const halda_model *model, const halda_fleets *fleets,
                                       const halda_partition_classes *classes, const int32_t *ks, int32_t n_k,
                                       halda_partition_classes_frontier *frontier);

int64_t halda_partition_classes_bytes(const int32_t *counts, int32_t n_classes, int32_t max_groups);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_PARTITION_CLASSES_H */
