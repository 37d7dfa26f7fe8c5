// Exact device selection under layer bounds (halda_solve_subsets_boxed, include/halda_subsets_boxed.h): the
// kernels that enumerate halda_solve_subsets' candidates and price each one under every box in one pass, and
// the pick over (box, fleet, d). Included by halda.hip after halda_sweep.hpp, whose pieces they join unedited:
// SubsetFleet / SubsetArgs and subset_kept_index (the combo enumeration and its one-ds_permute compaction),
// bounded_lane_at (fields and bounds gathered in one round trip) and bounded_fleet<Rec, kTables>.
//
// Items of one d. A candidate under a box is an item; a launch works on items [i0, i0 + n) of the d's numbering
// and keeps best_k / obj_value per item at its launch-local index. The order is fleet, then box, then candidate
// (candidate innermost):
//   register route (U.cmax > 0)  g = (f * n_box + b) * cmax + cand      -- cmax slots per group, slots past cnt idle
//   table and expansion routes   g = item_off[f] * n_box + b * cnt[f] + cand   -- compact
// so the (box, fleet) group the pick kernel reduces is one contiguous run, neighbouring waves read the same
// parent's field lines and the same plane lines, and a fleet's lines are finished with (all boxes, all
// candidates) before the next fleet's are touched: the live set in L2 is one parent and its planes, whatever the
// table's size or n_box. Box-major order would walk the whole table once per box.
#pragma once

// (fleet, group-relative item) of d-item g in the compact numbering: the last fleet whose first item is <= g,
// a binary search over uniform reads (fleets without candidates share their successor's offset and lose to it).
__device__ inline int subset_box_fleet(const SubsetArgs &U, int n_box, int64_t g) {
    int lo = 0, hi = U.n_fleets - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sload_i64(&U.fl[mid].item_off) * n_box <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One item on either fused route: the candidate's kept devices compacted onto the low lanes, lane j's device
// g = base + idx priced under plane b (a kept device carries the bounds of its PARENT index; a dropped device's
// bounds are never read), then bounded_fleet unedited -- the same code on the same fields and bounds as
// halda_sweep_subfleets_box[_tables]_kernel runs for item (fleet, kept list, b), hence the same bits. `slot` is
// the item's launch-local index (best_k / obj_value), `strip` its 64-entry w / n strip of the ring.
template <class Rec, bool kTables>
__device__ inline void subset_box_item(const SweepArgs &A, const SubsetArgs &U, const SubBoxArgs &X,
                                       const SubsetFleet &sf, int f, int b, int64_t cand, int64_t nd, int slot,
                                       int64_t strip, const WaveCtx &w, int lane) {
    const uint64_t combo = sload_u64(U.combos + sf.combo_off + cand);
    const int64_t base = sload_i64(A.F.dev_off + f);
    int nk;
    const int idx = subset_kept_index(sf.drop_mask, combo, sf.M, lane, &nk);
    const int64_t g = base + idx;
    bounded_fleet<Rec, kTables>(
        A, slot, w, Wave(lane),
        bounded_lane_at<std::is_same<Rec, BoxRec>::value>(A, X, lane, g, int64_t(b) * nd + g, strip * 64, nk));
}

// halda_sweep_subsets_box_kernel: the register route of one d -- one wave per (fleet, box, candidate),
// kSweepWavesPerBlock per workgroup, every fleet of M = A.uM + d devices; the host sends only batches the boxed
// entry's fused gate admits (plan_sweep's kRegAlone over (items, A.uM)) and n_fleets * n_box * cmax < 2^31 (two
// 32-bit divisions). The fleet record, the combo, the dev_off entry and the plane stride are wave-uniform reads
// through the scalar cache. The record type is the launch's, chosen once: a box record when an n array was
// passed, else a bound record. w / n go to a ring of 64-entry strips nobody reads (ring_mask).
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_subsets_box_kernel(
    SweepArgs A, SubsetArgs U, SubBoxArgs X, int n_box, int ring_mask) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    if (i >= U.n) return;
    const int lane = int(threadIdx.x & 63);
    const uint32_t g = uint32_t(U.i0) + uint32_t(i);
    const uint32_t grp = g / uint32_t(U.cmax);  // f * n_box + b
    const int cand = int(g - grp * uint32_t(U.cmax));
    const int f = int(grp / uint32_t(n_box)), b = int(grp - uint32_t(f) * uint32_t(n_box));
    const SubsetFleet sf = subset_fleet(U, f);
    if (cand >= sf.cnt) return;
    const int64_t nd = sload_i64(A.F.dev_off + X.table_fleets);
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    if (X.n_min || X.n_max) subset_box_item<BoxRec, false>(A, U, X, sf, f, b, cand, nd, i, i & ring_mask, w, lane);
    else subset_box_item<BoundRec, false>(A, U, X, sf, f, b, cand, nd, i, i & ring_mask, w, lane);
}

// halda_sweep_subsets_box_tables_kernel: the table route of one d -- one wave per workgroup on a persistent
// grid with the table kernel's LDS slice (plan_sweep's for the unbounded batch of the d's list shapes: it depends
// on no bound, so one slice serves every box), items dealt b, b + grid, ... in the compact numbering, fleets of
// mixed sizes 1 .. kK1MaxM, every k. The host sends fewer than 2^31 items per d (a 32-bit division). The
// record type is chosen outside the item loop (one loop per type). Each workgroup owns one
// strip of the ring.
template <class Rec>
__device__ inline void subset_box_tables(const SweepArgs &A, const SubsetArgs &U, const SubBoxArgs &X, int n_box,
                                         int ring_mask, unsigned char *smem) {
    const int lane = threadIdx.x;
    const WaveCtx w = wave_ctx(smem, make_slice(A.mmax, A.r1max, A.tab, A.tab_kc));
    const int64_t nd = sload_i64(A.F.dev_off + X.table_fleets);
    const int64_t strip = int64_t(blockIdx.x) & ring_mask;
    for (int64_t it = blockIdx.x; it < U.n; it += gridDim.x) {
        const int64_t g = U.i0 + it;
        const int f = subset_box_fleet(U, n_box, g);
        const SubsetFleet sf = subset_fleet(U, f);
        const uint32_t rem = uint32_t(g - sf.item_off * n_box);
        const uint32_t b = rem / uint32_t(sf.cnt);
        subset_box_item<Rec, true>(A, U, X, sf, f, int(b), int64_t(rem - b * uint32_t(sf.cnt)), nd, int(it), strip, w,
                                   lane);
    }
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_subsets_box_tables_kernel(
    SweepArgs A, SubsetArgs U, SubBoxArgs X, int n_box, int ring_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (X.n_min || X.n_max) subset_box_tables<BoxRec>(A, U, X, n_box, ring_mask, smem);
    else subset_box_tables<BoundRec>(A, U, X, n_box, ring_mask, smem);
}

// halda_subsets_box_index_kernel: the expansion route -- one wave per item of the compact numbering writes the
// candidate as an item of halda_solve_subfleets_boxed (parent, sub_off, the kept devices' parent indices, and
// its box) over the launch's items; U.l0 is the listed devices in front of item i0.
__global__ __launch_bounds__(256) void halda_subsets_box_index_kernel(SubsetArgs U, int n_box, int32_t *parent,
                                                                      int64_t *sub_off, int32_t *sub_idx,
                                                                      int32_t *item_box) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    if (i >= U.n) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t g = U.i0 + i;
    const int f = subset_box_fleet(U, n_box, g);
    const SubsetFleet sf = subset_fleet(U, f);
    const int64_t rem = g - sf.item_off * n_box;
    const int64_t b = rem / sf.cnt, cand = rem - b * sf.cnt;
    const uint64_t combo = sload_u64(U.combos + sf.combo_off + cand);
    int nk;
    const int idx = subset_kept_index(sf.drop_mask, combo, sf.M, lane, &nk);
    const int64_t so = sf.list_off * n_box + rem * int64_t(sf.M - U.d) - U.l0;
    if (lane < nk) sub_idx[so + lane] = idx;
    if (lane == 0) {
        parent[i] = f;
        item_box[i] = int32_t(b);
        sub_off[i] = so;
        if (i == U.n - 1) sub_off[i + 1] = so + nk;
    }
}

// halda_subsets_box_pick_kernel: one workgroup per (box, fleet) (blockIdx.y the box) -- halda_subsets_pick_kernel's
// lexicographic (obj_value, candidate index) arg-min with strict <, over the launch's items of the group (this
// d), folded into frontier point (box, fleet, d) only when strictly lower where the group began in an earlier
// launch (that launch's candidates come first). A group without candidates, or none feasible inside the box,
// reads INFEASIBLE, +inf, mask 0, best_k 0. No atomics, nothing shared between workgroups. stride: max_drop + 1.
__global__ __launch_bounds__(256) void halda_subsets_box_pick_kernel(SubsetArgs U, int n_box, const double *obj,
                                                                     const int32_t *best_k, SubsetFrontier R,
                                                                     int stride) {
    const int f = int(blockIdx.x), bx = int(blockIdx.y);
    const SubsetFleet sf = subset_fleet(U, f);
    const int64_t first = U.cmax > 0 ? (int64_t(f) * n_box + bx) * U.cmax : sf.item_off * n_box + int64_t(bx) * sf.cnt;
    const int64_t a = first > U.i0 ? first : U.i0;
    const int64_t e = first + sf.cnt, lim = U.i0 + U.n;
    const int64_t b = e < lim ? e : lim;
    const int64_t at = (int64_t(bx) * U.n_fleets + f) * stride + U.d;
    if (sf.cnt == 0) {
        if (threadIdx.x == 0 && U.i0 == 0) {
            R.status[at] = HALDA_STATUS_INFEASIBLE;
            R.obj[at] = kInf;
            R.dropped_mask[at] = 0;
            R.best_k[at] = 0;
        }
        return;
    }
    if (a >= b) return;
    double o = kInf;
    int64_t c = -1;
    for (int64_t g = a + threadIdx.x; g < b; g += 256) subset_min(o, c, obj[g - U.i0], g - first);
    for (int s = 32; s >= 1; s >>= 1) {
        const double o2 = __shfl_xor(o, s);
        const int64_t c2 = (int64_t(__shfl_xor(int(uint64_t(c) >> 32), s)) << 32) | uint32_t(__shfl_xor(int(c), s));
        subset_min(o, c, o2, c2);
    }
    __shared__ double so[4];
    __shared__ int64_t sc[4];
    if ((threadIdx.x & 63) == 0) {
        so[threadIdx.x >> 6] = o;
        sc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < 4; ++wv) subset_min(o, c, so[wv], sc[wv]);
    if (a > first && !(o < R.obj[at])) return;  // the group began earlier: only a strictly lower value moves it
    uint64_t mask = 0;
    if (o < kInf) {
        const uint64_t combo = U.combos[sf.combo_off + c];
        int r = 0;
        for (uint64_t m = sf.drop_mask; m; m &= m - 1, ++r)
            if ((combo >> r) & 1) mask |= m & (~m + 1);
    }
    R.status[at] = o < kInf ? HALDA_STATUS_OPTIMAL : HALDA_STATUS_INFEASIBLE;
    R.obj[at] = o;
    R.dropped_mask[at] = mask;
    R.best_k[at] = o < kInf ? best_k[first + c - U.i0] : 0;
}
