/*
 * halda.h — C ABI of libhalda, the MI355X (gfx950) solver for batches of
 * fixed-k HALDA MILPs.
 *
 * What it replaces. The reference (firstbatchxyz/distilp 0.1.6) solves one
 * fixed-k MILP per (fleet, k) with
 *     res = milp(c=c_obj, integrality=integrality, bounds=bounds,
 *                constraints=constraints, options=options)
 * at src/distilp/solver/halda_p_solver.py:340-346 (scipy 1.15.3 -> HiGHS
 * 1.8.0), and reads only res.success and res.x (:347-353). One call of
 * halda_solve_batch() stands in for a whole batch of such milp() calls: the
 * MILP arrives in CSR form exactly as scipy would hand it to HiGHS
 * (A = [A_ub ; A_eq], the ub rows in the reference's order then the single
 * equality row, scipy/optimize/_milp.py:60-71), and status/x come back per
 * instance with the same meaning as (res.success, res.x).
 *
 * The solve is exact (proven optimum, gap 0): libhalda validates that the CSR
 * has the HALDA structure (columns [w|n|s1|s2|s3|t|z|C], SURVEY.md appendix
 * A) and reduces it to a separable assignment problem that it solves by a
 * min-plus dynamic program over sum(w) on the GPU, with a cycle-time
 * threshold search when k > 1. A matrix without that structure is rejected
 * with HALDA_STATUS_UNSUPPORTED, never approximated.
 *
 * Ownership. Every pointer in halda_batch / halda_result is owned by the
 * caller. halda_solve_batch() takes HOST pointers, copies them to the device
 * and keeps nothing after it returns except grow-only scratch inside ctx.
 * halda_solve_batch_device() takes DEVICE pointers and is asynchronous on the
 * given HIP stream. Calls on one ctx must be serialised (from the host); the
 * work they enqueue on different streams runs concurrently (the per-launch
 * scratch is per stream), so independent batches may alternate over streams to
 * keep several in flight. Use one ctx per GPU.
 * Errors: functions return 0 on success and a negative code otherwise; the
 * message of the last failure on the calling thread is in halda_last_error().
 */
#ifndef HALDA_H
#define HALDA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALDA_ABI_VERSION 3

/* per-instance status (halda_result.status) */
#define HALDA_STATUS_OPTIMAL 0       /* res.success == True                   */
#define HALDA_STATUS_LIMIT 1         /* reserved (time/node limit)            */
#define HALDA_STATUS_INFEASIBLE 2    /* res.success == False (HiGHS status 2) */
#define HALDA_STATUS_UNSUPPORTED (-1) /* CSR is not a HALDA MILP              */
#define HALDA_STATUS_TOO_LARGE (-2)  /* exceeds the batch's shape summary     */

/* return codes */
#define HALDA_OK 0
#define HALDA_E_ARG (-22)
#define HALDA_E_HIP (-5)
#define HALDA_E_NODEV (-19)

typedef struct halda_batch {
    int32_t n_inst;
    /* Shape summary: upper bounds over the batch that size the on-chip (LDS)
     * scratch. With M = (n_cols-1)/7, W = equality rhs and R = W - sum_i lb(w_i)
     * (the layers left after every device's minimum), per instance:
     *   max_cols   >= n_cols
     *   max_R1     >= R + 1
     *   max_tab    >= M * (R + 1)   over instances with c[C] == 0 (k == 1)
     *   max_tab_kc >= M * (R + 1)   over instances with c[C]  > 0 (k  > 1)
     * halda_solve_batch() (host pointers) computes them itself when all are 0.
     * An instance exceeding them gets HALDA_STATUS_TOO_LARGE. No cap on R + 1 or M
     * beyond the int32 shape fields: instances whose tables exceed the LDS budget
     * are solved on global-memory tables (halda_solve_big_kernel). */
    int32_t max_cols;
    int32_t max_R1;
    int32_t max_tab;
    int32_t max_tab_kc;
    const int32_t *n_cols; /* [n_inst] N = 7M + 1 */
    const int32_t *n_rows; /* [n_inst] ub rows + 1 eq row */
    const int64_t *csr_off; /* [n_inst] start of the instance's row_ptr segment (n_rows + 1 entries) */
    const int64_t *col_off; /* [n_inst] start into c / col_lb / col_ub / integrality / x */
    const int64_t *row_off; /* [n_inst] start into row_lb / row_ub */
    const int32_t *row_ptr; /* absolute offsets into col_idx / val; instances of one fleet may share a segment */
    const int32_t *col_idx;
    const double *val;
    const double *c;
    const double *col_lb;
    const double *col_ub;
    const double *row_lb; /* -inf for ub rows */
    const double *row_ub;
    const uint8_t *integrality;
    double mip_rel_gap; /* accepted for API parity; the solve is exact */
    double mip_abs_gap;
    double time_limit;
    const double *x0; /* optional warm start, may be NULL (unused by the exact solver) */
    const double *y0;
} halda_batch;

typedef struct halda_result {
    int32_t *status;     /* [n_inst] HALDA_STATUS_* */
    double *x;           /* col_off layout, written for OPTIMAL instances */
    double *obj_lin;     /* [n_inst] c.x */
    double *dual_bound;  /* [n_inst] proven lower bound (== obj_lin when OPTIMAL) */
    double *gap;         /* [n_inst] relative gap (0 when OPTIMAL) */
    int64_t *nodes;      /* [n_inst] dynamic-programming passes evaluated */
} halda_result;

/* ABI version (HALDA_ABI_VERSION). */
int halda_version(void);

/* Bind a context to HIP device `device_ordinal` (must be gfx950). */
int halda_init(int device_ordinal, void **ctx);

/* Synchronous solve of a batch given in HOST memory (replaces a loop of milp() calls). */
int halda_solve_batch(void *ctx, const halda_batch *in, halda_result *out);

/* Asynchronous solve of a batch whose arrays are already in DEVICE memory (HBM),
 * enqueued on `stream` (a hipStream_t; NULL = the context's stream). */
int halda_solve_batch_device(void *ctx, const halda_batch *in, halda_result *out, void *stream);

/* halda_solve_batch_device with the caller's settled instances: settled[i] != 0
 * (a DEVICE array of n_inst bytes) states that the caller has already proved
 * instance i bound-infeasible (sum_j ceil(lb(w_j)) > W, e.g. M devices of w >= 1
 * over W = L/k < M layers: the k's milp() returns res.success == False,
 * halda_p_solver.py:369-436). Its result is written as HALDA_STATUS_INFEASIBLE
 * (the screen's own verdict for it: obj_lin = dual_bound = gap = inf, nodes 0)
 * and nothing of it but its flag is read. The batch has no screen launch: its
 * k = 1 kernel (halda_solve_k1_settled_kernel) writes the settled outputs and
 * screens every other instance on the way, with the screen's rules.
 * settled[i] == 0 instances are solved as by halda_solve_batch_device, bit for
 * bit; settled == NULL is halda_solve_batch_device. A settled flag on an
 * instance that is not infeasible is the caller's error (it is not checked). */
int halda_solve_batch_device_settled(void *ctx, const halda_batch *in, halda_result *out, const uint8_t *settled,
                                     void *stream);

/* Device time of the last solve's kernel sequence (both launches) in ms. */
int halda_last_kernel_ms(void *ctx, double *ms);

/* Device time of the last solve's general kernel (halda_solve_kernel) alone, in ms. */
int halda_last_solve_kernel_ms(void *ctx, double *ms);

/* Record the per-launch HIP events the *_ms queries read (on = 1, the default);
 * off drops four event records per launch from the stream. */
int halda_set_timing(void *ctx, int on);

/* Device time of the last solve per launch, in ms: ms3[0] the screen kernel
 * (halda_screen_kernel), ms3[1] the persistent k = 1 kernel (halda_solve_k1_kernel),
 * ms3[2] the general kernel's launches (k > 1, then k = 1 wide / hand-backs). A settled batch
 * (halda_solve_batch_device_settled) has no screen launch: ms3[0] = 0 and ms3[1] is its k = 1 kernel
 * (halda_solve_k1_settled_kernel, which screens on its way). */
int halda_last_phase_ms(void *ctx, double *ms3);

/* ------------------------------------------------------------------------
 * Whole k-sweeps on the GPU: lowering + solve + argmin over k.
 *
 * halda_solve_fleets() runs the reference's `halda_solve` for a batch of
 * fleets (halda_p_solver.py:369-436): per fleet it lowers every k-candidate
 * to the fixed-k MILP exactly as solve_fixed_k_milp does
 * (halda_p_solver.py:59-338 with the coefficients of dense_common.py:25-230,
 * same operation order, bit-identical CSR to the host lowering), solves them
 * with the kernels above and keeps the best k by the reference's rule
 * (ascending k, strict "<" on obj_value). Inputs are a flat table of the
 * device fields the formulas read (one entry per device, fleets contiguous),
 * so a stream of re-profiled fleets never goes through per-device Python
 * objects. obj_value = c.x + sum t_comm + sum xi + kappa is formed on the GPU
 * (c.x summed in a fixed tree order: within 1e-12 relative of NumPy's dot).
 * ------------------------------------------------------------------------ */

typedef struct halda_model {
    double f_q_b1;      /* ModelProfile.f_q["b_1"] (when has_f_q) */
    double f_out_b1;    /* ModelProfile.f_out["b_1"] (when has_f_out) */
    int32_t has_f_q, has_f_out;
    double b_prime;     /* b_prime(model, kv) (dense_common.py:25-46), an integer value */
    double b_layer, b_in, b_out, V;
    int32_t L;
} halda_model;

/* halda_fleets.flags bits, per device */
#define HALDA_DEV_HEAD 1       /* is_head */
#define HALDA_DEV_UMA 2        /* is_unified_mem */
#define HALDA_DEV_CPU_RATE 4   /* Q in scpu: scpu_b1 = scpu[Q]["b_1"] */
#define HALDA_DEV_GPU 8        /* a GPU FLOPs table and load throughput (beta is active) */
#define HALDA_DEV_GPU_RATE 16  /* ... and Q in that table: sgpu_b1 = table[Q]["b_1"] */
#define HALDA_DEV_CUDA_OK 32   /* has_cuda and d_avail_cuda is not None */
#define HALDA_DEV_METAL_OK 64  /* has_metal and d_avail_metal is not None */
#define HALDA_DEV_METAL_AVAIL 128 /* d_avail_metal is not None (M2 RAM row present) */

typedef struct halda_fleets {
    int32_t n_fleets;
    int32_t min_devices, max_devices; /* over the batch (size the scratch and the shape summary) */
    const int64_t *dev_off;           /* [n_fleets + 1]: fleet f owns devices dev_off[f] .. dev_off[f+1]-1 */
    const uint8_t *os_class;          /* 1 mac_no_metal (M1), 2 mac_metal (M2), 3 anything else (M3) */
    const uint8_t *flags;             /* HALDA_DEV_* */
    const double *scpu_b1, *sgpu_b1;  /* FLOP/s for batch 1 at quantization Q */
    const double *T_cpu, *T_gpu;      /* T_gpu: the load throughput matching the GPU table */
    const double *t_kvcpy_cpu, *t_kvcpy_gpu, *t_ram2vram, *t_vram2ram, *t_comm, *s_disk;
    /* byte counts: the profiles' integers as doubles (exact below 2^53 bytes; ABI 3 -- ABI 2 had int64) */
    const double *d_avail_ram, *c_cpu, *c_gpu, *d_avail_cuda, *d_avail_metal;
    const double *swap;               /* min(d_bytes_can_swap, d_swap_avail) for android, else 0 */
} halda_fleets;

typedef struct halda_fleet_result {
    int32_t *best_k;     /* [n_fleets] best k, 0 when no k is feasible */
    double *obj_value;   /* [n_fleets] */
    int32_t *w, *n;      /* [dev_off[n_fleets]] device layout */
    double *obj_by_k;    /* [n_fleets * n_k] obj_value per k (+inf infeasible); may be NULL */
    int32_t *status;     /* [n_fleets * n_k] HALDA_STATUS_* per k; may be NULL */
    double *x;           /* [n_fleets * n_k * (7 max_devices + 1)] x per (fleet, k), column layout; may be NULL */
    double *c;           /* same layout: the lowered objective c per (fleet, k); may be NULL */
    /* Optional compact x / c layout (ABI 2): x_off[f * n_k + j] = element offset of instance (f, k_j)'s
     * 7 M_f + 1 entries in x and c, or -1 for an instance whose x / c are not wanted (e.g. L / k < M_f,
     * which cannot be optimal). NULL: the dense layout above. Device memory for halda_solve_fleets,
     * host memory for halda_solve_fleets_host / _multi (x and c then hold max(x_off + 7 M_f + 1)). */
    const int64_t *x_off;
} halda_fleet_result;

/* Asynchronous on `stream` (NULL = the context's stream): the halda_fleets and
 * halda_fleet_result arrays are device memory; ks (host memory, n_k entries)
 * is ascending, unique, > 0 (at most 64 entries on the fused path). Shape limit:
 * (L / ks[0] - min_devices + 1) * max_devices <= 2^27; tables beyond the LDS budget go to HBM. */
int halda_solve_fleets(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                       int32_t n_k, halda_fleet_result *out, void *stream);

/* A prepared halda_solve_fleets for a table that stays resident (a streaming deployment re-solves the
 * same buffers as their contents change): the kernel choice, grids, LDS slices and kernel arguments are
 * derived from the shapes once, at creation, so each halda_fleets_plan_launch() is one or two kernel
 * enqueues on `stream` (NULL = the context's stream), asynchronous, with the results of a
 * halda_solve_fleets call on the same arguments. The device arrays behind `fleets` / `out` must stay
 * allocated with the same shapes (n_fleets, dev_off, min / max devices) while the plan lives; their
 * contents may change between launches. A halda_set_fleets_path on the context re-plans the plan at its
 * next launch. Launches of one context's plans must be serialised on the host, like every call on
 * that context. */
int halda_fleets_plan_create(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_fleet_result *out, void **plan);
int halda_fleets_plan_launch(void *plan, void *stream);
/* `steps` launches in one call, launch t of plans[(first + t) % n_plans] on streams[(first + t) %
 * n_streams] (a streaming caller's batches rotating over resident tables and streams, without a host
 * round trip per batch); stops at the first failing launch and returns its code. */
int halda_fleets_plan_launch_many(void *const *plans, int32_t n_plans, void *const *streams, int32_t n_streams,
                                  int64_t first, int32_t steps);
void halda_fleets_plan_free(void *plan);

/* A group of prepared plans run as a stream of batches: halda_fleets_group_launch(group, first, steps,
 * stream) solves batch t = plans[(first + t) % n_plans] for t = 0 .. steps - 1, each batch's results in
 * its own plan's arrays, exactly as halda_fleets_plan_launch_many(plans, n_plans, &stream, 1, first,
 * steps) would leave them. When every plan is a register sweep of one shape (the same model, k list,
 * fleet count and fleet size uM <= 64, no x / c outputs: C3's resident copies) the steps run as ONE
 * launch of one wave per (batch, fleet) item (steps <= 65,535); when every plan is a k-slot
 * sweep of one shape (fleets of <= 16 devices with k > 1 tables: C2) as one k-slot launch of one
 * workgroup per (batch, group of four fleets) item (steps <= 65,535), then one gated table launch for the
 * fleets they flagged (*persistent = 1); otherwise batch by batch on `stream` (*persistent = 0). The group copies what it
 * needs from the plans at creation (the plans may be freed after it); the tables and result arrays
 * behind them must stay allocated while the group lives. Plans and groups fail with HALDA_E_ARG once
 * their context was freed. Replaces the per-batch loop over halda_solve (halda_p_solver.py:369-436)
 * that a streaming caller runs. */
int halda_fleets_group_create(void *const *plans, int32_t n_plans, void **group, int32_t *persistent);
int halda_fleets_group_launch(void *group, int64_t first, int32_t steps, void *stream);
void halda_fleets_group_free(void *group);

/* How halda_solve_fleets runs (default 1; HALDA_FLEETS_PATH=csr / =wave at halda_init select 0 / 2):
 * 1 the fused sweep (halda_sweep_kernel: every (fleet, k) built in registers from the device
 *   fields, solved and compared in one wave per fleet; no MILP is materialised); batches of more
 *   than 64 fleets of at most 16 devices that need k > 1 tables run four fleets per wave, one per
 *   16-lane segment, and one wave per open k (halda_sweep_kslot_kernel: the best k picked in the
 *   workgroup), or, when its LDS does not fit (and at most 16 k), every k in turn in one wave
 *   (halda_sweep_seg_kernel);
 * 2 the fused sweep, one fleet per wave only;
 * 3 (test path) the fused sweep with every k = 1 solve of the register launch done by the exact DP
 *   that launch falls back to, never by its register greedy;
 * 4 the fused sweep with the segment kernel instead of the k-slot kernel;
 * 5 (test path) the fused sweep with the k-slot kernel's k = 2 threshold scan unsplit (path 1 splits
 *   it over two waves);
 * 6 (test path) the fused sweep with the k-slot kernel's split scan in sequential order (path 1 lets
 *   its part 1 take rows finite at both ends unchecked, the leaf checks and phase 0 made by other waves
 *   of the workgroup; here part 1 makes them itself, as it does for any other row);
 * 0 the CSR pipeline (lowering kernel -> the halda_solve_batch kernels -> pick kernel), which also
 *   keeps the lowered batch for halda_last_lowered. All give the same statuses and k, an optimal x
 *   of the same objective, and the same x wherever the optimum is unique; among several optimal
 *   plans (fleets with equal devices) the greedy and the DP may return different ones.
 * HALDA_E_ARG for any other path. */
int halda_set_fleets_path(void *ctx, int path);

/* Device time of the last halda_solve_fleets call per launch, in ms (per-launch events on, see
 * halda_set_timing; 0 for launches that did not run; ms8 holds 9 entries): ms8[0] the fused sweep kernel
 * (halda_sweep_kernel), ms8[7] the segment kernel (halda_sweep_seg_kernel), ms8[8] the k-slot kernel
 * (halda_sweep_kslot_kernel), ms8[1] their table launch (halda_sweep_tables_kernel / halda_sweep_big_kernel:
 * the flagged fleets, or the whole batch when k > 1 / wide fleets need tables from the start);
 * CSR pipeline: ms8[2] lowering, ms8[3] screen, ms8[4] k = 1 solve, ms8[5] general kernel,
 * ms8[6] pick. */
int halda_last_fleet_ms(void *ctx, double *ms8);

/* Synchronous variant on HOST arrays (halda_fleets / halda_fleet_result in host
 * memory; obj_by_k and status may be NULL). A one-fleet call (a single halda_solve) is answered by a
 * wave the context keeps resident on its own stream: it stays for up to 2 ms after each answer (or
 * until halda_resident_release / halda_free), and any device-wide wait of libhalda's HIP runtime
 * (hipDeviceSynchronize, hipFree) in that window waits for it. */
int halda_solve_fleets_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                            int32_t n_k, halda_fleet_result *out);

/* ------------------------------------------------------------------------
 * Sub-fleets of a resident table: leave-one-out and what-if.
 *
 * An item is (parent fleet f of `table`, index list s): s holds local device indices into fleet f, each
 * in [0, M_f), in any order, repeats allowed. Its meaning is the fleet [devs_f[j] for j in s], in that
 * order (so kappa's head is the first listed device with HALDA_DEV_HEAD, else the first listed device),
 * and every output of item i equals, bit for bit, what halda_solve_fleets writes for fleet i of a table
 * that holds the listed devices materialised. `out` is an ordinary halda_fleet_result over the items:
 * best_k / obj_value per item, w / n laid out by sub_off, obj_by_k / status per (item, k), x / c dense
 * with the items' max_devices or compact through x_off over (item, k).
 *
 * Two routes, one contract (halda_set_subfleets_path). When every item has the same length M' <= 64 and
 * a batch of n_items fleets of M' devices would run as the register sweep alone (no table launch), one
 * wave per item reads its index list and gathers its devices' fields straight from the parent table
 * (halda_sweep_subfleets_kernel): no expanded table exists. Every other call first copies the listed
 * devices into a compact table in context scratch (halda_expand_subfleets_kernel; grow-only, 130 bytes
 * per listed device) and runs halda_solve_fleets on it.
 * ------------------------------------------------------------------------ */
typedef struct halda_subfleets {
    int32_t n_items;
    int32_t min_devices, max_devices;   /* over the items' list lengths */
    const int32_t *parent;              /* [n_items] fleet of the table */
    const int64_t *sub_off;             /* [n_items + 1], sub_off[0] = 0 */
    const int32_t *sub_idx;             /* [sub_off[n_items]] local device indices within the parent */
} halda_subfleets;

/* Asynchronous on `stream` (NULL = the context's stream); table, items and out hold device arrays, ks is
 * host memory as for halda_solve_fleets. A parent or device index out of range, an empty list, a
 * sub_off[0] != 0 or list lengths outside [min_devices, max_devices] are the caller's error (not checked,
 * as settled flags are not). With mixed list lengths the call reads sub_off[n_items] back to size its
 * scratch (it waits for `stream` once). */
int halda_solve_subfleets(void *ctx, const halda_model *model, const halda_fleets *table,
                          const halda_subfleets *items, const int32_t *ks, int32_t n_k, halda_fleet_result *out,
                          void *stream);

/* Synchronous variant on HOST arrays: only the parent table and the item arrays cross PCIe on the way in.
 * Validates the items (parent and device indices in range, no empty list, sub_off ascending from 0, the
 * length summary, which must be the lists' shortest and longest length exactly: the dense x / c layout
 * strides by max_devices) and returns HALDA_E_ARG with a message in halda_last_error otherwise;
 * min_devices = max_devices = 0 lets it compute the summary itself. It knows sub_off[n_items], so it
 * never reads it back. */
int halda_solve_subfleets_host(void *ctx, const halda_model *model, const halda_fleets *table,
                               const halda_subfleets *items, const int32_t *ks, int32_t n_k,
                               halda_fleet_result *out);

/* Which route the context's last halda_solve_subfleets / _host call took: 1 the fused route
 * (halda_sweep_subfleets_kernel), 2 the expansion route, 0 when none ran yet. */
int halda_last_subfleets_route(void *ctx, int *route);

/* How halda_solve_subfleets runs: 0 automatic (default: the fused route where it applies), 1 always
 * expand (test path: the fused route is compared against it). HALDA_E_ARG for any other path. */
int halda_set_subfleets_path(void *ctx, int path);

/* ------------------------------------------------------------------------
 * Model variants of one table: which KV precision and context length can this fleet serve?
 *
 * halda_solve_variants solves one fleet table for n_var models in one call. The packed table does not
 * depend on the variant (it reads the model's quantization and whether f_q / f_out carry "b_1"), so
 * the variants must share L, has_f_q and has_f_out; every other field (b_prime -- kv_bits and n_kv --,
 * b_layer, b_in, b_out, V, f_q_b1, f_out_b1) is per variant. Outputs are variant-major: with
 * nf = n_fleets and nd = dev_off[nf], best_k / obj_value hold n_var * nf entries (variant v, fleet f at
 * v * nf + f), w / n hold n_var * nd (variant v's block at v * nd), obj_by_k / status n_var * nf * n_k,
 * x / c are dense with stride 7 max_devices + 1 over (v, f, k), or compact through an x_off of
 * n_var * nf * n_k entries (element offsets into the one x / c, -1: not wanted). Slice v of every output
 * equals, bit for bit, what halda_solve_fleets(ctx, &models[v], fleets, ks, n_k, ...) writes.
 *
 * Two routes, one contract (halda_set_variants_path). Where halda_solve_fleets would run one launch in
 * which a wave owns a fleet from start to end -- the register sweep alone over fleets of one size <= 64
 * (halda_sweep_variants_kernel), or a small batch's table kernel alone (at most 64 fleets, whatever
 * n_var: halda_sweep_tables_variants_kernel) -- the variants run as ONE launch, blockIdx.y the variant,
 * each wave reading its variant's model from a per-call array in context scratch. Every other shape
 * (gated launches, the k-slot and segment kernels, global tables, more than 64 k, the CSR pipeline) is
 * a loop of n_var halda_solve_fleets calls on the caller's stream with the output pointers moved.
 * ------------------------------------------------------------------------ */

/* Asynchronous on `stream` (NULL = the context's stream); models and ks are host memory, fleets and out
 * hold device arrays. HALDA_E_ARG (nothing launched) when n_var < 1 or n_var > 65535, or when the models
 * do not all share L, has_f_q and has_f_out. On the loop route a call with n_var > 1 reads
 * dev_off[n_fleets] back to place the w / n slices (it waits for `stream` once). */
int halda_solve_variants(void *ctx, const halda_model *models, int32_t n_var, const halda_fleets *fleets,
                         const int32_t *ks, int32_t n_k, halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe once on the way in, the n_var result slices
 * on the way out. It knows dev_off[n_fleets], so it never reads it back. */
int halda_solve_variants_host(void *ctx, const halda_model *models, int32_t n_var, const halda_fleets *fleets,
                              const int32_t *ks, int32_t n_k, halda_fleet_result *out);

/* Which route the context's last halda_solve_variants / _host call took: 1 fused (one launch), 2 the
 * per-variant loop, 0 when none ran yet. */
int halda_last_variants_route(void *ctx, int *route);

/* How halda_solve_variants runs: 0 automatic (default: the fused route where it applies), 1 always loop
 * (test path: the fused route is compared against it). HALDA_E_ARG for any other path. */
int halda_set_variants_path(void *ctx, int path);

/* ------------------------------------------------------------------------
 * A deployed plan priced on the fleet as it is now: evaluate, regret, keep or move.
 *
 * A plan for fleet f of M devices is (k[f], w[M], n[M]) (w / n in the table's device layout). Under
 * `model` it is evaluated at W = L / k on the device records the sweep builds. It is feasible when
 * k > 0, sum w = W, every 1 <= w_i <= W, every n_i lies in the interval its capacity rows leave at w_i
 * (0 <= n_i <= min(w_i, nhi) with nhi = W on a device with a usable GPU, else 0, narrowed by the VRAM
 * and the class-3 RAM row), no integer slack exceeds its bound, and no record is rejected. Its
 * objective is then sum_i g_i + (k - 1) C + the fleet's constants, with the least integer slacks at
 * (w_i, n_i), g_i the device's cost, H_i its least cycle time and C = max(0, max_i H_i): for the
 * (best_k, w, n) a halda_solve_fleets call returned, the obj_value that call returned (bit for bit on
 * fleets of at most 64 devices against the one-fleet-per-wave sweep; within 1e-12 relative otherwise).
 *
 * Per fleet: status HALDA_STATUS_OPTIMAL (feasible), _INFEASIBLE, or _UNSUPPORTED (a record the sweep
 * would reject, or W >= 1e6); obj_value and cycle (C) are +inf unless feasible; bottleneck is the
 * lowest device index with H_i = max H, -1 when not feasible or max H <= 0; reason is a bit mask:
 *    1  sum w != W                         2  some w_i outside [1, W]
 *    4  some n_i outside its interval (n_i > 0 without a usable GPU, n_i > w_i, ...)
 *    8  a slack over its bound (the class-1 / class-2 RAM slack at w_i, or the VRAM slack at n_i)
 *   16  record rejected                   32  k <= 0: "no plan" (nothing else is looked at)
 * Bits 4 and 8 are looked at on the devices whose w_i is in range. Bit 32 lets a sweep's own
 * best_k / w / n be fed back as the plan even for fleets where no k was feasible.
 * x / c (optional) hold the plan's 7 M + 1 columns [w|n|s1|s2|s3|t|z|C] as the sweep's x / c hold
 * them for a solved k (c[C] = k - 1), zeros for a plan that is not feasible: dense with stride
 * 7 max_devices + 1 per fleet, or compact through an x_off of n_fleets element offsets (-1: not
 * written).
 * ------------------------------------------------------------------------ */
typedef struct halda_plans {
    const int32_t *k;      /* [n_fleets] */
    const int32_t *w, *n;  /* [dev_off[n_fleets]] device layout */
} halda_plans;

typedef struct halda_plan_result {
    int32_t *status;     /* [n_fleets] HALDA_STATUS_* */
    double *obj_value;   /* [n_fleets] */
    double *cycle;       /* [n_fleets]; may be NULL */
    int32_t *bottleneck; /* [n_fleets]; may be NULL */
    int32_t *reason;     /* [n_fleets]; may be NULL */
    double *x, *c;       /* may be NULL */
    const int64_t *x_off; /* [n_fleets] or NULL (dense) */
} halda_plan_result;

/* Asynchronous on `stream` (NULL = the context's stream); every array is device memory. One launch
 * (halda_eval_plans_kernel: one wave per fleet, any fleet size). The plan arrays are only read: they
 * may be the best_k / w / n arrays an earlier halda_solve_fleets on the same stream wrote. */
int halda_eval_plans(void *ctx, const halda_model *model, const halda_fleets *fleets, const halda_plans *plans,
                     halda_plan_result *out, void *stream);

/* Synchronous variant on HOST arrays (x_off host memory too). */
int halda_eval_plans_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const halda_plans *plans,
                          halda_plan_result *out);

/* The k-sweep of the table and the evaluation of the incumbent plans in one call: `out` equals, bit for
 * bit, what halda_solve_fleets writes, `eval_out` what halda_eval_plans writes. Two routes, one contract
 * (halda_set_plans_path). By default the call runs halda_eval_plans and then halda_solve_fleets on
 * `stream` (any shape). On path 2, where the sweep is the register launch alone over fleets of one size
 * <= 64 (the sub-fleet and variants kernels' gate), it is ONE launch (halda_sweep_plans_kernel: each wave
 * prices its fleet's plan on the fields it loads for the sweep, so the table is read once); measured 7 %
 * ahead of the two launches on 4,096 fleets of 64 devices, inside the box-to-box spread, hence not the
 * default. This entry writes the sweep's outputs: plan arrays that alias
 * out->best_k / w / n are the caller's error here (not checked). */
int halda_solve_fleets_plans(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_plans *plans, halda_plan_result *eval_out,
                             halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe once for both. */
int halda_solve_fleets_plans_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                                  int32_t n_k, const halda_plans *plans, halda_plan_result *eval_out,
                                  halda_fleet_result *out);

/* Which route the context's last halda_solve_fleets_plans / _host call took: 1 fused (one launch), 2 the
 * evaluation launch then the sweep, 0 when none ran yet. */
int halda_last_plans_route(void *ctx, int *route);

/* How halda_solve_fleets_plans runs: 0 automatic (default: two launches), 1 always two launches, 2 the
 * fused route where it applies (two launches elsewhere). HALDA_E_ARG for any other path. */
int halda_set_plans_path(void *ctx, int path);

/* ------------------------------------------------------------------------
 * The k-sweep within per-device layer bounds: caps, pins and bounded moves.
 *
 * Two optional int32 arrays in the table's device layout narrow the w columns of every (fleet, k)
 * instance from [1, W] to [lo_i, hi_i], W = L / k:
 *    lo_i = max(1, w_min_i)   (a zero-filled array, or w_min == NULL: no lower bound)
 *    hi_i = min(W, w_max_i)   (INT32_MAX, or w_max == NULL: no upper bound)
 * The same arrays apply to every k of the call (a caller with a move budget around an incumbent passes
 * the incumbent's k alone). The answer is that of the reference's fixed-k MILP with only the bounds of
 * the w columns replaced: n, the slacks, z, C and every row are as in halda_solve_fleets, the other
 * devices' n are re-optimised, a device with lo = hi is pinned in w only, and the best k is picked by
 * the same rule (ascending k, strict "<"). An instance is HALDA_STATUS_INFEASIBLE when sum lo > W
 * (without bounds: M > W), when some lo_i > hi_i, or when sum hi < W; W >= 1e6 and rejected records
 * stay HALDA_STATUS_UNSUPPORTED. With no bounds, or with bounds that never bind (w_min <= 1,
 * w_max >= W), every output equals halda_solve_fleets' bit for bit. Bounds on n: halda_box, below.
 * ------------------------------------------------------------------------ */
typedef struct halda_bounds {
    const int32_t *w_min, *w_max; /* [dev_off[n_fleets]] device layout; either may be NULL */
} halda_bounds;

/* Asynchronous on `stream` (NULL = the context's stream); every array is device memory (ks: host).
 * Writes into `out` exactly the fields halda_solve_fleets writes. Two routes, one contract
 * (halda_set_bounds_path). General route (every shape): the batch is lowered on the GPU
 * (halda_lower_kernel), halda_bound_cols_kernel overwrites the w columns' bounds, and the CSR pipeline
 * solves it. Fused route: where the sweep is the register launch alone over fleets of one size <= 64
 * (the sub-fleet, variants and plans kernels' gate: no k > 1 has L / k >= M, and L - M + 1 <= 64 at
 * k = 1), ONE launch of halda_sweep_bounds_kernel, one wave per fleet. Table route (path 3 only, where
 * the fused route does not apply): any mix of fleets of 1 .. 64 devices, at most 64 k, whose unbounded
 * table slice fits the LDS budget -- small fleets, k > 1 with room -- in ONE launch of
 * halda_sweep_bounds_tables_kernel, one wave per fleet on that slice; nothing is handed back and no
 * context scratch is used. Bounds that never bind give the table sweep's bits there. */
int halda_solve_fleets_bounded(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                               int32_t n_k, const halda_bounds *bounds, halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays (x_off host memory too): the table and the bounds cross PCIe once. */
int halda_solve_fleets_bounded_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                                    int32_t n_k, const halda_bounds *bounds, halda_fleet_result *out);

/* Which route the context's last halda_solve_fleets_bounded / _boxed / _host call took: 1 fused (one launch),
 * 2 general (lowering, bounds, CSR pipeline), 3 the table route (one launch), 0 when none ran yet. */
int halda_last_bounds_route(void *ctx, int *route);

/* How halda_solve_fleets_bounded runs: 0 automatic, 1 always general, 2 the fused route where it
 * applies (general elsewhere), 3 the fused route where it applies, else the table route where it
 * applies (path 3; general elsewhere). HALDA_E_ARG for any other path. */
int halda_set_bounds_path(void *ctx, int path);

/* ------------------------------------------------------------------------
 * Layer bounds on n too: cap, pin or disable a device's GPU share (halda_solve_fleets_boxed).
 *
 * halda_box is halda_bounds with two more optional int32 arrays in the same layout, for the n columns.
 * Device i has the reference's own range n in [0, nhi_i], nhi_i = W on a GPU device, else 0:
 *    nlo_i  = max(0, n_min_i)      (zero, a negative entry, or n_min == NULL: no lower bound)
 *    nhi'_i = min(nhi_i, n_max_i)  (INT32_MAX, or n_max == NULL: no upper bound; 0: the GPU is not used)
 * The link row n_i <= w_i stays, so the effective lower bound on w is lo_i = max(1, w_min_i, nlo_i) -- an
 * implied bound of the same MILP, used in the sum lo > W verdict and in R = W - sum lo. The answer is
 * that of the reference's fixed-k MILP with only the bounds of the w and n columns replaced: every row
 * stays, and the slack, z and C columns keep their bounds -- the VRAM slack's upper bound stays nhi_i,
 * n_max narrows n, not the slack. An instance is HALDA_STATUS_INFEASIBLE in halda_solve_fleets_bounded's
 * three cases (with the folded lo_i) and when some nlo_i > nhi'_i (n_min_i >= 1 on a device without a GPU
 * included), in the same order of precedence against HALDA_STATUS_UNSUPPORTED. A device with
 * w_min = w_max and n_min = n_max is pinned in both columns: pinning every device prices that plan, with
 * halda_eval_plans' status and objective.
 *
 * With n_min and n_max both NULL the call IS halda_solve_fleets_bounded: the same route, the same
 * kernels, the same bits. With n arrays that never bind (n_min <= 0, n_max >= W) every output equals
 * that call's bit for bit. The routes, halda_set_bounds_path and halda_last_bounds_route are shared:
 * with n bounds the general route patches the lowered batch with halda_box_cols_kernel (w and n
 * columns), the fused route launches halda_sweep_box_kernel and the table route
 * halda_sweep_box_tables_kernel, each under the gate of its bounded twin.
 * ------------------------------------------------------------------------ */
typedef struct halda_box {
    const int32_t *w_min, *w_max, *n_min, *n_max; /* [dev_off[n_fleets]] device layout; any may be NULL */
} halda_box;

/* Asynchronous on `stream`; arguments and outputs as halda_solve_fleets_bounded (box == NULL: no bounds). */
int halda_solve_fleets_boxed(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_box *box, halda_fleet_result *out, void *stream);

/* Synchronous variant on HOST arrays, as halda_solve_fleets_bounded_host. */
int halda_solve_fleets_boxed_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                                  int32_t n_k, const halda_box *box, halda_fleet_result *out);

/* Many boxes on one table (n_box planes of halda_box's arrays, one launch): include/halda_boxes.h. */

/* A total move budget around a deployed plan: the best plan within B moved layers, and its frontier.
 *
 * The problem is the fixed-k MILP at the incumbent's k (one k per call, W = L / k) with the optional w_min /
 * w_max of halda_bounds on the w columns and ONE added constraint that couples the devices:
 * sum_i |w_i - w0_i| <= B. n, the slacks, z and C are re-optimised freely. Both plans sum to W, so
 * sum |delta| is even; the call works in p = sum_i max(0, w_i - w0_i), the layers that change device, and
 * answers every p = 0 .. max_p (B = 2 p) at once: point p is the optimum over the plans with
 * sum max(0, delta) <= p, and among equal objectives the plan with the fewest moves. The frontier is
 * non-increasing in p; point 0 is "w pinned, n re-optimised".
 *
 * Per point: status HALDA_STATUS_OPTIMAL, _INFEASIBLE (no plan within the budget and the bounds) or
 * _UNSUPPORTED (W >= 1e6, a rejected record, or -- device entry only -- an incumbent with w0_i < 1 or
 * sum w0 != W, which the host entry rejects with HALDA_E_ARG before any GPU work); obj the reference's
 * c.x + sum t_comm + sum xi + kappa (+inf where not optimal), the bits halda_eval_plans gives the returned
 * plan; moved = sum |w - w0| of the returned plan (<= 2 p); w and n as max_p + 1 planes in the table's device
 * layout (zeros where not optimal).
 *
 * Gate, from the shapes alone: every fleet has 1 .. 64 devices, 0 <= max_p <= 63, and
 * halda_budget_lds_bytes(max_devices, max_p, k) is at most 160 KiB. Outside it the call returns HALDA_E_ARG
 * and launches nothing: there is no fallback. One launch of halda_sweep_budget_kernel (one wave per fleet;
 * no context scratch, nothing shared between waves, so launches on different streams need no ordering). */
typedef struct halda_budget {
    const int32_t *w0;            /* [dev_off[n_fleets]] the incumbents' layer counts, device layout */
    const int32_t *w_min, *w_max; /* as halda_bounds; either may be NULL */
    int32_t max_p;                /* P = B / 2 */
} halda_budget;

typedef struct halda_frontier {
    int64_t n_devices; /* dev_off[n_fleets]: the stride of the w / n planes */
    int32_t *status;   /* [n_fleets * (max_p + 1)] */
    double *obj;       /* [n_fleets * (max_p + 1)] */
    int32_t *moved;    /* [n_fleets * (max_p + 1)] */
    int32_t *w, *n;    /* [(max_p + 1) * n_devices]: plane p holds point p's plan of every fleet */
} halda_frontier;

/* Asynchronous on `stream`; fleets, budget and frontier hold device arrays. */
int halda_solve_fleets_budget(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                              const halda_budget *budget, halda_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays (frontier->n_devices is taken from dev_off). */
int halda_solve_fleets_budget_host(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                                   const halda_budget *budget, halda_frontier *frontier);

/* Bytes of dynamic LDS per wave of halda_sweep_budget_kernel for this shape (the gate's figure); -1 for
 * max_devices < 1, max_p < 0 or k < 1. No context needed. */
int64_t halda_budget_lds_bytes(int32_t max_devices, int32_t max_p, int32_t k);

/* ------------------------------------------------------------------------
 * Re-placement of a live fleet after a device is lost or joins: the exact frontier.
 *
 * An item is a sub-fleet of a parent fleet in halda_subfleets' format (the listed devices in list order,
 * kappa's head by halda_solve_subfleets' rule) with the layers each listed device holds now: w0_i >= 0,
 * 0 for a device that holds nothing (a joiner). One k per call, W = L / k. The deficit D = W - sum w0 >= 0
 * is the number of layers the lost devices held. With delta_i = w_i - w0_i, loaded = sum max(0, delta) is
 * what some device must newly load and released = sum max(0, -delta) what is taken off a listed device;
 * loaded = D + released for every plan. Point p = 0 .. max_p is the optimum of the list's fixed-k problem
 * (what halda_solve_subfleets solves for it at that one k, inside the optional w_min / w_max) over the plans
 * with released <= p, among equal objectives the plan with the fewest released layers; n, the slacks, z and C
 * are re-optimised. The frontier is non-increasing; point 0 deals the orphans out and disturbs no survivor.
 * With D = 0 and every w0_i >= 1 the outputs are halda_solve_fleets_budget's of the materialised list, bit
 * for bit (moved = loaded + released).
 *
 * Per point: status HALDA_STATUS_OPTIMAL, _INFEASIBLE (no plan: with D = 0 and a joiner point 0 has none,
 * since every listed device needs w >= 1) or _UNSUPPORTED (W >= 1e6, a rejected record, or -- device entry
 * only -- some w0_i < 0, D < 0 or D > max_deficit, which the host entry rejects with HALDA_E_ARG before any
 * GPU work); obj as halda_frontier's (the bits halda_eval_plans gives the returned plan on the materialised
 * list; +inf where not optimal); loaded / released of the returned plan (zero where not optimal); w and n as
 * max_p + 1 planes laid out by sub_off (zeros where not optimal).
 *
 * Gate, from the shapes alone: lists of 1 .. 64 devices, 0 <= max_p <= 63, max_deficit >= 0,
 * 2 max_p + max_deficit <= 254, and halda_change_lds_bytes(max_devices, max_p, max_deficit, k) at most
 * 160 KiB. Outside it the call returns HALDA_E_ARG and launches nothing: there is no fallback. One launch of
 * halda_sweep_change_kernel (one wave per item; no context scratch, nothing shared between waves). */
typedef struct halda_change {
    const int32_t *w0;            /* [sub_off[n_items]] the layers each listed device holds, laid out by sub_off */
    const int32_t *w_min, *w_max; /* as halda_bounds, laid out by sub_off; either may be NULL */
    int32_t max_p;                /* P: the most released layers asked for */
    int32_t max_deficit;          /* an upper bound of every item's D (host entry: -1 = compute it) */
} halda_change;

typedef struct halda_change_frontier {
    int64_t n_devices; /* sub_off[n_items]: the stride of the w / n planes */
    int32_t *status;   /* [n_items * (max_p + 1)] */
    double *obj;       /* [n_items * (max_p + 1)] */
    int32_t *loaded;   /* [n_items * (max_p + 1)] */
    int32_t *released; /* [n_items * (max_p + 1)] */
    int32_t *w, *n;    /* [(max_p + 1) * n_devices]: plane p holds point p's plan of every item */
} halda_change_frontier;

/* Asynchronous on `stream`; table, items, change and frontier hold device arrays. The items are the
 * caller's to get right, as for halda_solve_subfleets (min_devices / max_devices must be the lists' shortest
 * and longest length). */
int halda_solve_change(void *ctx, const halda_model *model, const halda_fleets *table, const halda_subfleets *items,
                       int32_t k, const halda_change *change, halda_change_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays (frontier->n_devices is taken from sub_off). Validates the items as
 * halda_solve_subfleets_host does, every w0_i >= 0 and 0 <= D <= max_deficit per item; max_deficit = -1 lets
 * it take the items' largest D. */
int halda_solve_change_host(void *ctx, const halda_model *model, const halda_fleets *table,
                            const halda_subfleets *items, int32_t k, const halda_change *change,
                            halda_change_frontier *frontier);

/* Bytes of dynamic LDS per wave of halda_sweep_change_kernel for this shape (the gate's figure); -1 for
 * max_devices < 1, max_p < 0, max_deficit < 0 or k < 1. No context needed. */
int64_t halda_change_lds_bytes(int32_t max_devices, int32_t max_p, int32_t max_deficit, int32_t k);

/* ------------------------------------------------------------------------
 * Exact device selection: the best sub-fleet over all subsets of the droppable devices.
 *
 * Per fleet of M <= 64 devices: keep_mask names the devices that may not be dropped (bit i: device i;
 * NULL: none), q = M - |keep| are droppable, and a candidate is the fleet without d of them, the kept
 * devices in their order (kappa's head by halda_solve_subfleets' rule). A candidate's value is what
 * halda_solve_subfleets writes for that list, bit for bit (+inf where no k is feasible). Candidates are
 * enumerated by d ascending and, within one d, by their ascending dropped-index lists in lexicographic
 * order; among equal objectives the earliest wins (strict <).
 *
 * The frontier has max_drop + 1 points per fleet, laid out [fleet][max_drop + 1]: point d is the best
 * candidate with exactly d devices dropped -- status HALDA_STATUS_OPTIMAL or _INFEASIBLE, obj, the dropped
 * devices as a mask, and the candidate's best_k. A point whose candidates are all infeasible has +inf and
 * mask 0. A fleet may drop at most min(q, M - 1) devices: its points beyond that have no candidate and read
 * INFEASIBLE, +inf, mask 0, best_k 0 (so fleets of several sizes share one max_drop).
 *
 * Gate, from the shapes alone, before any GPU work (HALDA_E_ARG): every fleet has 1 .. 64 devices;
 * 0 <= max_drop <= 63 and max_drop <= min(q, M - 1) of at least one fleet; no keep bit at or above M; and
 * halda_subsets_count(q, min(max_drop, q, M - 1)) <= HALDA_SUBSETS_MAX candidates per fleet.
 *
 * Routes, per d (halda_last_subsets_route): fused -- every fleet of one size M and a batch of all the d's
 * candidates, fleets of M - d devices, planned as the register sweep alone (halda_solve_subfleets' gate):
 * one wave per (fleet, candidate) forms the candidate from a per-(q, d) combo list and gathers its
 * devices' fields from the table (halda_sweep_subsets_kernel); expansion -- every other shape:
 * halda_subsets_index_kernel writes the candidates as halda_solve_subfleets items in context scratch and
 * that entry's expansion route runs on them, in chunks of at most 2^21 listed devices. Either way
 * halda_subsets_pick_kernel reduces each (fleet, d) group on the device: the per-candidate values never
 * leave it. The scratch is per context, so the call runs after the previous user of the context's shared
 * scratch on another stream.
 * ------------------------------------------------------------------------ */
#define HALDA_SUBSETS_MAX (1 << 20)

typedef struct halda_subsets {
    int32_t max_drop;
    const uint64_t *keep_mask; /* HOST memory, [n_fleets], or NULL */
} halda_subsets;

typedef struct halda_subset_frontier {
    int32_t *status;        /* [n_fleets * (max_drop + 1)] */
    double *obj;            /* [n_fleets * (max_drop + 1)] */
    uint64_t *dropped_mask; /* [n_fleets * (max_drop + 1)] */
    int32_t *best_k;        /* [n_fleets * (max_drop + 1)] */
} halda_subset_frontier;

/* Asynchronous on `stream` (NULL = the context's stream); fleets and frontier hold device arrays, ks and
 * keep_mask are host memory. With mixed fleet sizes the call reads dev_off back (it waits for `stream`
 * once). */
int halda_solve_subsets(void *ctx, const halda_model *model, const halda_fleets *fleets, const halda_subsets *subsets,
                        const int32_t *ks, int32_t n_k, halda_subset_frontier *frontier, void *stream);

/* Synchronous variant on HOST arrays: the table crosses PCIe on the way in, the frontier on the way back. */
int halda_solve_subsets_host(void *ctx, const halda_model *model, const halda_fleets *fleets,
                             const halda_subsets *subsets, const int32_t *ks, int32_t n_k,
                             halda_subset_frontier *frontier);

/* sum over d <= max_drop of C(q, d), saturated at INT64_MAX; -1 for q < 0, q > 64 or max_drop < 0. No
 * context needed. */
int64_t halda_subsets_count(int32_t q, int32_t max_drop);

/* Which routes the context's last halda_solve_subsets / _host call took: 1 fused for every d, 2 expansion
 * for every d, 3 mixed (they differ by d), 0 when none ran yet. */
int halda_last_subsets_route(void *ctx, int *route);

/* How halda_solve_subsets runs: 0 automatic (default: the fused route where it applies), 1 always expand
 * (test path: the fused route is compared against it). HALDA_E_ARG for any other path. */
int halda_set_subsets_path(void *ctx, int path);

/* ------------------------------------------------------------------------
 * Scale-in and scale-out: WHICH devices to drop (or, from a pool, to add) under a released-layer budget.
 *
 * Per fleet of M <= 64 devices: w0_i >= 0 are the layers each device holds now (a pool device that has not
 * joined holds 0; sum w0 <= W = L / k), keep_mask names the devices that may not be dropped. A candidate is
 * halda_solve_subsets' -- the fleet without d of its q droppable devices, the kept devices in their order,
 * one 64-bit combo over droppable slots, enumerated by d ascending, then by ascending dropped-index lists in
 * lexicographic order. Its value at point p is exactly what halda_solve_change writes for that list with w0
 * (and w_min / w_max) restricted to it; its deficit is W - sum of the kept devices' w0.
 *
 * The frontier is a grid [fleet][d - min_drop][p], min_drop <= d <= max_drop, 0 <= p <= max_p: each cell is
 * the candidate with exactly d drops whose point p has the least raw objective, the earliest among equals
 * (strict <). Per cell: status HALDA_STATUS_OPTIMAL or _INFEASIBLE, obj, the dropped devices as a mask,
 * loaded / released of the winner's point p, and its plan w / n indexed by PARENT device (64 entries per cell,
 * 0 for a dropped device and past M). A (fleet, d) without a candidate (d > min(q, M - 1)), or a cell where no
 * candidate has a plan at p, reads INFEASIBLE, +inf, mask 0, zero counts and a zero plan.
 * Scale-out is the same call: the parent is the fleet followed by the pool, keep_mask the whole fleet, the
 * pool's w0 zero; "add a of the q pool devices" is d = q - a.
 *
 * Gate, from the shapes and w0 alone, before any GPU work (HALDA_E_ARG; there is no fallback): every fleet has
 * 1 .. 64 devices; 0 <= min_drop <= max_drop <= 63 and min_drop <= min(q, M - 1) of at least one fleet; no
 * keep bit at or above M; at most HALDA_SUBSETS_MAX candidates per fleet over the d range; every w0_i >= 0 and
 * sum w0 <= W; 0 <= max_p <= 63; and for every d in range that has a candidate, halda_solve_change's gate with
 * that d's longest list and largest deficit Dmax_d (halda_change_subsets_max_deficit over the fleets that
 * admit d): 2 max_p + Dmax_d <= 254 and halda_change_lds_bytes(len_d, max_p, Dmax_d, k) <= 160 KiB.
 *
 * One halda_solve_change launch per (d, chunk), each with its d's list lengths and max_deficit = Dmax_d (a
 * small d is not gated by a large d's deficit): halda_change_subsets_index_kernel writes the chunk's
 * candidates as items with their w0 / w_min / w_max in context scratch, halda_sweep_change_kernel runs on
 * them, halda_change_subsets_pick_kernel folds the chunk into the grid and copies each new winner's plan.
 * Chunks are cut at candidate boundaries so that halda_change_subsets_launch_bytes of a launch stays within
 * the context's cap (256 MiB; halda_set_change_subsets_chunk), one candidate at the least. The scratch is per
 * context, so the call runs after the previous user of the context's shared scratch on another stream.
 * ------------------------------------------------------------------------ */
typedef struct halda_change_subsets {
    const int32_t *w0;            /* [dev_off[n_fleets]] per parent device, laid out by dev_off */
    const int32_t *w_min, *w_max; /* as halda_bounds, per parent device; either may be NULL */
    int32_t min_drop, max_drop;   /* the d range */
    int32_t max_p;                /* P: the most released layers asked for */
    const uint64_t *keep_mask;    /* HOST memory, [n_fleets], or NULL */
} halda_change_subsets;

typedef struct halda_change_subset_frontier {
    int32_t *status;        /* [n_fleets * D1 * (max_p + 1)], D1 = max_drop - min_drop + 1 */
    double *obj;            /* the same extent */
    uint64_t *dropped_mask; /* the same extent */
    int32_t *loaded;        /* the same extent */
    int32_t *released;      /* the same extent */
    int32_t *w, *n;         /* [n_fleets * D1 * (max_p + 1) * 64], by parent device */
} halda_change_subset_frontier;

/* Asynchronous on `stream` (NULL = the context's stream) once the gate is formed: fleets, w0 / w_min / w_max
 * and frontier hold device arrays, keep_mask is host memory; the call reads dev_off and w0 back for the gate
 * (it waits for `stream`). */
int halda_solve_change_subsets(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                               const halda_change_subsets *subsets, halda_change_subset_frontier *frontier,
                               void *stream);

/* Synchronous variant on HOST arrays: the table and w0 / w_min / w_max cross PCIe on the way in, the grid on
 * the way back. */
int halda_solve_change_subsets_host(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                                    const halda_change_subsets *subsets, halda_change_subset_frontier *frontier);

/* The largest deficit of a fleet's candidates with d drops: W - sum w0 plus the d largest droppable w0 (w0:
 * HOST memory, M entries). -1 for M outside 1 .. 64, d < 0, a keep bit at or above M, or d beyond the
 * droppable devices. No context needed. */
int64_t halda_change_subsets_max_deficit(const int32_t *w0, int32_t M, uint64_t keep_mask, int32_t d, int32_t W);

/* Scratch bytes of one launch of n_items candidates of `len` listed devices at max_p: the items, the three
 * int arrays, the four per-point arrays and the two planes, plus a fixed 4096 for alignment. -1 for len < 1,
 * max_p < 0 or n_items < 0. No context needed. */
int64_t halda_change_subsets_launch_bytes(int32_t len, int32_t max_p, int64_t n_items);

/* The byte cap of one launch's scratch (test hook): 0 restores the default of 256 MiB; a launch always holds
 * at least one candidate. HALDA_E_ARG for a negative value. */
int halda_set_change_subsets_chunk(void *ctx, int64_t bytes);

/* Ask the context's resident wave (above) to leave now and wait until it has (a no-op when none
 * runs); the next one-fleet call relaunches it. For callers about to synchronise the whole device. */
int halda_resident_release(void *ctx);

/* Page-locked host memory for halda_solve_fleets_host's arrays. When EVERY array of the call's fleets and
 * results (and x_off) lies in blocks from halda_host_alloc, a call above the zero-copy size copies straight
 * between them and device memory (one DMA per array) instead of staging both ways through the context's
 * own pinned buffer with host memcpys -- the batch API packs its fleet table into such a block
 * (distilp_amd/solver/fleets.py). The results are the same either way. */
int halda_host_alloc(size_t bytes, void **ptr);
void halda_host_free(void *ptr);

/* Several GPUs from one process: a context per device (ordinals may repeat), and
 * halda_solve_fleets_host over all of them -- the fleets are dealt out in contiguous blocks, one host
 * thread per device, results written at each block's offsets. Fleets are independent, so no
 * collective is involved; multi-process / multi-node callers use one halda_init context per rank
 * (distilp_amd/distributed.py: torch.distributed / RCCL around it). */
int halda_init_multi(int n_dev, const int *ordinals, void **mctx);
int halda_solve_fleets_multi(void *mctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, halda_fleet_result *out);
void halda_free_multi(void *mctx);

/* Latency mode across processes, one per GPU: the ranks of an RCCL communicator
 * (ncclComm_t, passed as void*) each sweep their share of the k-candidates of every fleet --
 * ks[rank], ks[rank + world], ... -- on their own GPU (halda_solve_fleets), then agree on each fleet's
 * best k by the reference's rule (smallest obj_value, ties to the smallest k, halda_p_solver.py:407)
 * with device-side all-reduces over xGMI: MIN of obj_value, MIN of the k reaching it, SUM of the owner's
 * (w, n), and MIN / MAX of obj_by_k / status when those are requested. Every rank ends with the same
 * halda_fleet_result (device arrays; x and c must be NULL). Asynchronous on `stream`; every rank calls
 * it with the same fleets and ks. obj_value is the GPU-formed objective (see halda_solve_fleets).
 * halda_comm_unique_id / halda_comm_init / halda_comm_destroy wrap ncclGetUniqueId / ncclCommInitRank
 * (the 128-byte id goes from one rank to the others by any channel) for callers without their own
 * communicator. */
int halda_comm_unique_id(void *id128);
int halda_comm_init(void **comm, int world, int rank, const void *id128, int device_ordinal);
void halda_comm_destroy(void *comm);
int halda_solve_fleets_sharded(void *ctx, void *comm, const halda_model *model, const halda_fleets *fleets,
                               const int32_t *ks, int32_t n_k, halda_fleet_result *out, void *stream);

/* Latency mode's exact step sequence for `world` virtual ranks (1..16) on ONE device, for tests and
 * measurement where a node's GPUs are not available: every virtual rank's sub-sweep and shard kernels run
 * into its own result arrays (library scratch), and each RCCL all-reduce of halda_solve_fleets_sharded is
 * replaced, in the same order, by one device kernel reducing over the virtual ranks' arrays (MIN / SUM /
 * MAX as there). The arrays of virtual rank `report_rank` are the caller's `out`. Asynchronous on
 * `stream`. */
int halda_solve_fleets_sharded_emulated(void *ctx, int32_t world, int32_t report_rank, const halda_model *model,
                                        const halda_fleets *fleets, const int32_t *ks, int32_t n_k,
                                        halda_fleet_result *out, void *stream);

/* The lowered batch of the last halda_solve_fleets call (device pointers into ctx
 * scratch, valid until the next call on ctx): for tests and diagnostics. An
 * instance with L / k < M (bound-infeasible) carries only its header, w bounds,
 * c[C] and equality-row bounds. x / c of halda_fleet_result are 0 for every
 * instance that is not OPTIMAL. */
int halda_last_lowered(void *ctx, halda_batch *lowered, halda_result *solved);

/* Bytes of dynamic LDS per wave of the general kernel's larger launch for a batch of this shape. */
int64_t halda_lds_bytes(int32_t max_cols, int32_t max_R1, int32_t max_tab, int32_t max_tab_kc);

/* Copy the calling thread's last error message into buf. Returns its length. */
int halda_last_error(char *buf, size_t len);

void halda_free(void *ctx);

#ifdef __cplusplus
}
#endif

#endif /* HALDA_H */
