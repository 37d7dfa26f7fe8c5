// halda_rank.hpp -- device selection and scale-in / scale-out for fleets of up to 256 devices
// (halda_solve_subsets_wide, halda_solve_change_subsets_wide; included by halda.hip behind halda_sweep.hpp).
//
// The wave routes carry a candidate as a 64-bit combo the host enumerates. Here a candidate is a RANK: its index
// in the enumeration order of its (fleet, d) group -- ascending dropped-slot lists, lexicographic -- and the GPU
// unranks it by the combinatorial number system. No combo list exists: the host uploads one RankFleet per
// (d, fleet) and, once per call, the table of binomials C(n, j), n <= 256, j <= 63, saturated above 2^20
// (a gated call never reads a saturated entry: every count it meets is that of a subset of one group's
// candidates, and a group has at most 2^20).
//
// Unranking, one wave, all state wave-uniform: position j of the combination, with `start` the least slot still
// free, dd = d - j slots still to choose of qp = q - start, takes slot start + c for the largest c whose
// "combinations that begin below it", C(qp, dd) - C(qp - c, dd), is at most the rank left. The 64 lanes test 64
// consecutive c at once against the launch's rows of the table in LDS and a ballot counts the prefix that
// holds: at most four steps for 256 slots, no loop over ranks. The chosen slots are four 64-bit words.
// Slots are the droppable devices in ascending order, so a parent device is dropped when it is droppable and the
// number of droppable devices below it is a chosen slot; the wave covers 256 parent devices in four passes of
// ballots, and kept device t lands at t - #{dropped < t}.
//
// House rules as everywhere: no atomics, no spin-waits, nothing shared between workgroups, vector stores only.
#pragma once

constexpr int kRankMaxM = 256;                   // devices per fleet: four passes of one wave
constexpr int kRankMaxD = 63;                    // dropped devices per candidate
constexpr uint32_t kRankSat = (1u << 20) + 1;    // the table's "more than 2^20"
constexpr int kRankTableW = kRankMaxM + 1;       // global table: row j = C(0 .. 256, j), j = 0 .. kRankMaxD
constexpr int kRankMaxP1 = 128;                  // frontier points per item on the wide change route

struct RankFleet {       // 64 bytes, read through the scalar cache
    int64_t item_off;    // the fleet's first item of this d (compact prefix over the fleets)
    int64_t list_off;    // listed devices of every item in front of the fleet's first
    uint64_t drop[4];    // its droppable devices, bit t & 63 of word t >> 6
    int32_t cnt;         // its candidates of this d (0: d is beyond what the fleet may drop)
    int32_t M;           // its devices
    int32_t q;           // its droppable devices
    int32_t pad;
};

struct RankArgs {
    const RankFleet *fl;    // [n_fleets] of this d
    const uint32_t *binom;  // the call's table, [kRankMaxD + 1][kRankTableW]
    int64_t i0;             // the launch's first item
    int64_t l0;             // listed devices in front of item i0
    int32_t n;              // its items
    int32_t n_fleets, d;
    int32_t qmax;           // the most droppable devices of a fleet: the LDS rows hold n = 0 .. qmax
};

struct RankSlots {  // the chosen slots of a candidate, wave-uniform
    uint64_t m0, m1, m2, m3;
};

extern __shared__ uint32_t rank_rows[];  // rows 1 .. d of the table, qmax + 1 entries each

__device__ inline RankFleet rank_fleet(const RankArgs &U, int f) {
    const int64_t *p = reinterpret_cast<const int64_t *>(U.fl + f);
    RankFleet s;
    s.item_off = sload_i64(p);
    s.list_off = sload_i64(p + 1);
    s.drop[0] = uint64_t(sload_i64(p + 2));
    s.drop[1] = uint64_t(sload_i64(p + 3));
    s.drop[2] = uint64_t(sload_i64(p + 4));
    s.drop[3] = uint64_t(sload_i64(p + 5));
    const int64_t cm = sload_i64(p + 6), qp = sload_i64(p + 7);
    s.cnt = int32_t(uint32_t(uint64_t(cm)));
    s.M = int32_t(uint64_t(cm) >> 32);
    s.q = int32_t(uint32_t(uint64_t(qp)));
    s.pad = 0;
    return s;
}

// The fleet of item g: the last one whose item_off is <= g (a binary search over uniform reads).
__device__ inline int rank_fleet_of(const RankArgs &U, int64_t g) {
    int lo = 0, hi = U.n_fleets - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sload_i64(&U.fl[mid].item_off) <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Every thread of the workgroup: rows 1 .. d of the call's table into LDS, then one barrier.
__device__ inline void rank_load_rows(const RankArgs &U) {
    const int w = U.qmax + 1, tot = U.d * w;
    for (int e = int(threadIdx.x); e < tot; e += int(blockDim.x)) {
        const int j = e / w;
        rank_rows[e] = U.binom[(j + 1) * kRankTableW + (e - j * w)];
    }
    __syncthreads();
}

__device__ inline uint64_t rank_word(const RankSlots &s, int w) {
    return w == 0 ? s.m0 : w == 1 ? s.m1 : w == 2 ? s.m2 : s.m3;
}

// The d slots of rank r among the C(q, d) ascending lists of q slots, lexicographic. The whole wave calls it
// with uniform arguments; r < C(q, d).
__device__ inline RankSlots rank_unrank(int w, int q, int d, uint32_t r, int lane) {
    RankSlots s{0, 0, 0, 0};
    int start = 0;
    for (int j = 0; j < d; ++j) {
        const int dd = d - j, qp = q - start, cmax = qp - dd;
        const uint32_t *row = rank_rows + (dd - 1) * w;
        const uint32_t top = uint32_t(__builtin_amdgcn_readfirstlane(int(row[qp])));
        int c = 0;
        for (int step = 0; step < 4; ++step) {
            const int cc = step * 64 + lane + 1;
            const bool in = cc <= cmax;
            const uint32_t below = top - row[in ? qp - cc : qp];  // combinations that begin below start + cc
            const int t = __popcll(__ballot(in && below <= r));
            c += t;
            if (t < 64) break;
        }
        r -= top - uint32_t(__builtin_amdgcn_readfirstlane(int(row[qp - c])));
        const int v = start + c, wv = v >> 6;
        const uint64_t bit = uint64_t(1) << (v & 63);
        s.m0 |= wv == 0 ? bit : 0;
        s.m1 |= wv == 1 ? bit : 0;
        s.m2 |= wv == 2 ? bit : 0;
        s.m3 |= wv == 3 ? bit : 0;
        start = v + 1;
    }
    return s;
}

// Pass `pass` of the wave over the parent devices, t = 64 pass + lane: is device t dropped by the chosen slots?
// slots_below: the droppable devices of the passes in front.
__device__ inline bool rank_dropped(uint64_t word, int slots_below, const RankSlots &s, int lane) {
    const int slot = slots_below + __popcll(word & ((uint64_t(1) << lane) - 1));
    return ((word >> lane) & 1) && ((rank_word(s, slot >> 6) >> (slot & 63)) & 1);
}

// halda_rank_index_kernel / halda_change_rank_index_kernel: one wave per candidate of the launch's items
// [i0, i0 + n) of one d. The wave unranks its candidate and writes it as an item of the entry behind it --
// parent, sub_off and the kept devices' indices in parent order -- and, for scale-in (kChange), beside them the
// kept devices' w0 / w_min / w_max gathered from the per-parent-device arrays.
template <bool kChange>
__device__ inline void rank_index_item(const RankArgs &U, const ChangeSubsetsSrc &G, const ChangeSubsetsItems &O) {
    rank_load_rows(U);
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    if (i >= U.n) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t g = U.i0 + i;
    const int f = rank_fleet_of(U, g);
    const RankFleet sf = rank_fleet(U, f);
    const int64_t cand = g - sf.item_off;
    const RankSlots sl = rank_unrank(U.qmax + 1, sf.q, U.d, uint32_t(cand), lane);
    const int64_t so = sf.list_off + cand * int64_t(sf.M - U.d) - U.l0;
    int64_t base = 0;
    if (kChange) base = sload_i64(G.dev_off + f);
    int slots_below = 0, gone_below = 0;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        if (pass * 64 >= sf.M) break;
        const int t = pass * 64 + lane;
        const uint64_t word = sf.drop[pass];
        const bool gone = rank_dropped(word, slots_below, sl, lane);
        const uint64_t gm = __ballot(gone);
        if (t < sf.M && !gone) {
            const int64_t at = so + t - gone_below - __popcll(gm & ((uint64_t(1) << lane) - 1));
            O.sub_idx[at] = t;
            if (kChange) {
                O.w0[at] = G.w0[base + t];
                if (G.w_min) O.w_min[at] = G.w_min[base + t];
                if (G.w_max) O.w_max[at] = G.w_max[base + t];
            }
        }
        slots_below += __popcll(word);
        gone_below += __popcll(gm);
    }
    if (lane == 0) {
        O.parent[i] = f;
        O.sub_off[i] = so;
        if (i == U.n - 1) O.sub_off[i + 1] = so + (sf.M - U.d);
    }
}

__global__ __launch_bounds__(256) void halda_rank_index_kernel(RankArgs U, ChangeSubsetsItems O) {
    rank_index_item<false>(U, ChangeSubsetsSrc{}, O);
}

__global__ __launch_bounds__(256) void halda_change_rank_index_kernel(RankArgs U, ChangeSubsetsSrc G,
                                                                      ChangeSubsetsItems O) {
    rank_index_item<true>(U, G, O);
}

// The winner's dropped devices, ascending, into out[0 .. d), and -1 into out[d .. dcap): the whole wave, one
// pass per 64 parent devices. ok false: nothing was chosen, all of out reads -1.
__device__ inline void rank_write_dropped(const RankFleet &sf, const RankSlots &sl, bool ok, int d, int dcap, int lane,
                                          int32_t *out) {
    int slots_below = 0, gone_below = 0;
    if (ok) {
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            if (pass * 64 >= sf.M) break;
            const uint64_t word = sf.drop[pass];
            const bool gone = rank_dropped(word, slots_below, sl, lane);
            const uint64_t gm = __ballot(gone);
            if (gone) out[gone_below + __popcll(gm & ((uint64_t(1) << lane) - 1))] = pass * 64 + lane;
            slots_below += __popcll(word);
            gone_below += __popcll(gm);
        }
    }
    if (lane >= (ok ? d : 0) && lane < dcap) out[lane] = -1;
}

// halda_rank_pick_kernel: halda_subsets_pick_kernel's reduction on (objective, rank) -- one workgroup per
// fleet, the arg-min of the launch's items of the fleet's group (this d), lexicographic with strict <, so the
// earliest candidate among equal objectives; folded into the frontier entry where the group began in an earlier
// launch only for a strictly lower value. Wave 0 then unranks the winner once and writes its dropped device
// indices. A group without candidates, or whose candidates are all infeasible, gets INFEASIBLE, +inf, no index.
struct RankFrontier {
    int32_t *status;
    double *obj;
    int32_t *dropped;  // [fleet][stride][dcap], -1 padded
    int32_t *best_k;
};

__global__ __launch_bounds__(256) void halda_rank_pick_kernel(RankArgs U, const double *obj, const int32_t *best_k,
                                                              RankFrontier R, int stride, int dcap) {
    rank_load_rows(U);
    const int f = int(blockIdx.x);
    const int lane = int(threadIdx.x & 63);
    const RankFleet sf = rank_fleet(U, f);
    const int64_t a = sf.item_off > U.i0 ? sf.item_off : U.i0;
    const int64_t e = sf.item_off + sf.cnt, lim = U.i0 + U.n;
    const int64_t b = e < lim ? e : lim;
    const int64_t at = int64_t(f) * stride + U.d;
    if (sf.cnt == 0) {
        if (threadIdx.x < 64 && U.i0 == 0) {
            if (lane < dcap) R.dropped[at * dcap + lane] = -1;
            if (lane == 0) {
                R.status[at] = HALDA_STATUS_INFEASIBLE;
                R.obj[at] = kInf;
                R.best_k[at] = 0;
            }
        }
        return;
    }
    if (a >= b) return;
    double o = kInf;
    int64_t c = -1;
    for (int64_t g = a + threadIdx.x; g < b; g += 256) subset_min(o, c, obj[g - U.i0], g - sf.item_off);
    for (int s = 32; s >= 1; s >>= 1) {
        const double o2 = __shfl_xor(o, s);
        const int64_t c2 = (int64_t(__shfl_xor(int(uint64_t(c) >> 32), s)) << 32) | uint32_t(__shfl_xor(int(c), s));
        subset_min(o, c, o2, c2);
    }
    __shared__ double so[4];
    __shared__ int64_t sc[4];
    if (lane == 0) {
        so[threadIdx.x >> 6] = o;
        sc[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    o = so[0];
    c = sc[0];
    for (int wv = 1; wv < 4; ++wv) subset_min(o, c, so[wv], sc[wv]);
    if (a > sf.item_off && !(o < R.obj[at])) return;  // the group began earlier: only a strictly lower value moves it
    const bool ok = o < kInf;
    const uint32_t r = uint32_t(__builtin_amdgcn_readfirstlane(int(c)));
    const RankSlots sl = rank_unrank(U.qmax + 1, sf.q, ok ? U.d : 0, r, lane);
    rank_write_dropped(sf, sl, ok, U.d, dcap, lane, R.dropped + at * dcap);
    if (lane == 0) {
        R.status[at] = ok ? HALDA_STATUS_OPTIMAL : HALDA_STATUS_INFEASIBLE;
        R.obj[at] = o;
        R.best_k[at] = best_k[sf.item_off + c - U.i0];
    }
}

// halda_change_rank_pick_kernel: halda_change_subsets_pick_kernel's reduction on (raw objective, rank) -- one
// workgroup per fleet for the launch's d; per point p the arg-min of the launch's items of the fleet's group,
// the four waves' results through LDS behind one workgroup barrier. Then wave v takes the points v, v + 4, ...:
// a cell whose group began in an earlier launch moves only for a strictly lower value; the wave unranks the
// cell's winner, writes its dropped indices and, in four passes, the winner's point-p plan by parent device
// (256 entries per cell, 0 for a dropped device and past M), read from the chunk's planes at the device's
// position among the kept.
struct ChangeRankGrid {
    int32_t *status;
    double *obj;
    int32_t *dropped;  // [cell][dcap], -1 padded
    int32_t *loaded, *released;
    int32_t *w, *n;    // [cell][kRankMaxM]
};

__global__ __launch_bounds__(256) void halda_change_rank_pick_kernel(RankArgs U, ChangeSubsetsChunk C,
                                                                     ChangeRankGrid R, int dcap) {
    rank_load_rows(U);
    const int f = int(blockIdx.x);
    const RankFleet sf = rank_fleet(U, f);
    const int lane = int(threadIdx.x & 63), wv = int(threadIdx.x >> 6);
    const int P1 = C.P1;
    const int64_t at = (int64_t(f) * C.D1 + (U.d - C.d0)) * P1;
    if (sf.cnt == 0) {
        if (U.i0 == 0)
            for (int p = wv; p < P1; p += 4) {
                if (lane < dcap) R.dropped[(at + p) * dcap + lane] = -1;
                if (lane == 0) {
                    R.status[at + p] = HALDA_STATUS_INFEASIBLE;
                    R.obj[at + p] = kInf;
                    R.loaded[at + p] = 0;
                    R.released[at + p] = 0;
                }
                for (int t = lane; t < kRankMaxM; t += 64) {
                    R.w[(at + p) * kRankMaxM + t] = 0;
                    R.n[(at + p) * kRankMaxM + t] = 0;
                }
            }
        return;
    }
    const int64_t a = sf.item_off > U.i0 ? sf.item_off : U.i0;
    const int64_t e = sf.item_off + sf.cnt, lim = U.i0 + U.n;
    const int64_t b = e < lim ? e : lim;
    if (a >= b) return;
    __shared__ double so[4][kRankMaxP1];
    __shared__ int64_t sc[4][kRankMaxP1];
    for (int p = 0; p < P1; ++p) {
        double o = kInf;
        int64_t c = -1;
        for (int64_t g = a + threadIdx.x; g < b; g += 256) subset_min(o, c, C.obj[(g - U.i0) * P1 + p], g - sf.item_off);
        for (int s = 32; s >= 1; s >>= 1) {
            const double o2 = __shfl_xor(o, s);
            const int64_t c2 = (int64_t(__shfl_xor(int(uint64_t(c) >> 32), s)) << 32) | uint32_t(__shfl_xor(int(c), s));
            subset_min(o, c, o2, c2);
        }
        if (lane == 0) {
            so[wv][p] = o;
            sc[wv][p] = c;
        }
    }
    __syncthreads();
    const bool first = a == sf.item_off;
    for (int p = wv; p < P1; p += 4) {
        double o = so[0][p];
        int64_t c = sc[0][p];
        for (int v = 1; v < 4; ++v) subset_min(o, c, so[v][p], sc[v][p]);
        if (!first && !(o < R.obj[at + p])) continue;  // the group began earlier: only a strictly lower value moves it
        const bool ok = o < kInf;
        const uint32_t r = uint32_t(__builtin_amdgcn_readfirstlane(int(c)));
        const RankSlots sl = rank_unrank(U.qmax + 1, sf.q, ok ? U.d : 0, r, lane);
        rank_write_dropped(sf, sl, ok, U.d, dcap, lane, R.dropped + (at + p) * dcap);
        const int64_t src0 = int64_t(p) * C.nd + sf.list_off + c * int64_t(sf.M - U.d) - U.l0;
        int slots_below = 0, gone_below = 0;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int t = pass * 64 + lane;
            const uint64_t word = pass * 64 < sf.M ? sf.drop[pass] : 0;
            const bool gone = rank_dropped(word, slots_below, sl, lane);
            const uint64_t gm = __ballot(gone);
            int wl = 0, nl = 0;
            if (ok && t < sf.M && !gone) {
                const int64_t src = src0 + t - gone_below - __popcll(gm & ((uint64_t(1) << lane) - 1));
                wl = C.w[src];
                nl = C.n[src];
            }
            R.w[(at + p) * kRankMaxM + t] = wl;
            R.n[(at + p) * kRankMaxM + t] = nl;
            slots_below += __popcll(word);
            gone_below += __popcll(gm);
        }
        if (lane == 0) {
            const int64_t it = (sf.item_off + c - U.i0) * P1 + p;
            R.status[at + p] = ok ? HALDA_STATUS_OPTIMAL : HALDA_STATUS_INFEASIBLE;
            R.obj[at + p] = o;
            R.loaded[at + p] = ok ? C.loaded[it] : 0;
            R.released[at + p] = ok ? C.released[it] : 0;
        }
    }
}
