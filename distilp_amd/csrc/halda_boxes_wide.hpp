// halda_boxes_wide.hpp -- the boxed k-sweep beyond one wave (halda_solve_fleets_boxes_wide).
// Included by halda.hip after halda_sweep.hpp: the records, the splits, table_pass and the workgroup reduction
// (WideRed) are that header's, called as they stand.
//
// halda_sweep_boxes_wide_kernel: the fixed-k MILP of §4.6 under a box (w_min, w_max and the optional n_min,
// n_max; n_i <= w_i stays) for every k of the call and every (box, fleet) item, on one 256-thread workgroup per
// item: fleets of up to 256 devices, any R = W - sum wlo whose two value planes fit the LDS.
//   LDS        two value planes of S = max R + 1 doubles (state s = layers handed out above sum wlo), two row
//              buffers of kBoxRowBuf doubles per table (the DP's current chunk and the next one in flight), per
//              device wlo, the reduction slots, the per-k objectives.
//   workspace  (the workgroup's slice of the context's global tables) G and, for k > 1, H as rows of R + 1
//              doubles; one arg-min uint16 per (device, state), read only at backtrack time; the plan row (table
//              indices) and its n.
// No record is formed here that the box kernels do not form: field_rec, bound_src, table_entry (through
// table_pass), split_full and dev_cycle are called, not copied.
#pragma once

constexpr int kBoxRowBuf = kWideThreads;  // a row chunk: one entry per thread
constexpr int kBoxNone = 65535;           // an arg-min entry: unreached

struct BoxesWideSlice {
    int64_t V, rowG, rowH, wlo, red, pick, lds;  // LDS offsets, and the LDS total
    int64_t G, H, arg, plan, nplan, global;      // workspace offsets, and the workspace total
    int S;
};

// The slice of a launch whose widest fleet has max_devices devices and whose longest row has max_R + 1 entries.
__host__ __device__ inline BoxesWideSlice boxes_wide_slice(int max_devices, int max_R, bool any_k_gt_1) {
    BoxesWideSlice s;
    const int64_t S = int64_t(max_R) + 1, M = max_devices;
    s.S = int(S);
    int64_t o = 0;
    s.V = o;     o = align16(o + 2 * S * 8);
    s.rowG = o;  o = align16(o + 2 * int64_t(kBoxRowBuf) * 8);
    s.rowH = o;  o = align16(o + (any_k_gt_1 ? 2 * int64_t(kBoxRowBuf) * 8 : 0));
    s.wlo = o;   o = align16(o + M * 4);
    s.red = o;   o = align16(o + 2 * kWideWaves * 8);
    s.pick = o;  o = align16(o + 64 * 8);
    s.lds = o;
    o = 0;
    s.G = o;     o = align16(o + M * S * 8);
    s.H = o;     o = align16(o + (any_k_gt_1 ? M * S * 8 : 0));
    s.arg = o;   o = align16(o + M * S * 2);
    s.plan = o;  o = align16(o + M * 2);
    s.nplan = o; o = align16(o + M * 4);
    s.global = o;
    return s;
}

struct BoxesWideCtx {
    double *V, *rowG, *rowH, *pick;  // LDS
    int *wlo;
    double *G, *H;                   // workspace
    uint16_t *arg, *plan;
    int *nplan;
    int S, mmax;
};

__device__ inline BoxesWideCtx boxes_wide_ctx(unsigned char *smem, unsigned char *work, const BoxesWideSlice &sl,
                                              int mmax) {
    BoxesWideCtx c;
    c.V = reinterpret_cast<double *>(smem + sl.V);
    c.rowG = reinterpret_cast<double *>(smem + sl.rowG);
    c.rowH = reinterpret_cast<double *>(smem + sl.rowH);
    c.pick = reinterpret_cast<double *>(smem + sl.pick);
    c.wlo = reinterpret_cast<int *>(smem + sl.wlo);
    c.G = reinterpret_cast<double *>(work + sl.G);
    c.H = reinterpret_cast<double *>(work + sl.H);
    c.arg = reinterpret_cast<uint16_t *>(work + sl.arg);
    c.plan = reinterpret_cast<uint16_t *>(work + sl.plan);
    c.nplan = reinterpret_cast<int *>(work + sl.nplan);
    c.S = sl.S;
    c.mmax = mmax;
    return c;
}

// One DP over the M devices: new[s] = min_e cur[s - e] + G_i[e] in ascending e with a strict "<" (the least w_i
// wins), the entries with !(H_i[e] <= T) masked (kc == 0: no mask). Thread t owns states t, t + 256, ... A
// device's row reaches the inner loop through LDS in chunks of kBoxRowBuf entries, ascending: while the threads
// run chunk (i, ch) on one row buffer, thread e holds entry e of the next chunk -- of the same row, or the first of
// device i + 1 -- in registers and stores it into the other buffer before the step's one barrier. A state's
// running minimum over the chunks of a row stays in its slot of the new plane (its own thread's). Every thread
// reads the same row entry at a time (a broadcast). kArg: the step also stores its arg-min plane (the scan's
// value passes need none). Returns F_M[R], the same bits on every thread; the planes are free on return.
template <bool kArg>
__device__ inline double boxes_wide_dp(const BoxesWideCtx &c, int M, int R1, double kc, double T, int tid) {
    double *cur = c.V, *nxt = c.V + c.S;
    for (int s = tid; s < R1; s += kWideThreads) cur[s] = s == 0 ? 0.0 : kInf;
    const int nch = (R1 + kBoxRowBuf - 1) / kBoxRowBuf;
    if (tid < R1) {
        c.rowG[tid] = c.G[tid];
        if (kc > 0.0) c.rowH[tid] = c.H[tid];
    }
    __syncthreads();
    int b = 0;
    for (int i = 0; i < M; ++i) {
        uint16_t *ai = c.arg + int64_t(i) * R1;
        for (int ch = 0; ch < nch; ++ch) {
            const bool last = ch + 1 == nch;
            const int ni = last ? i + 1 : i, ne = (last ? 0 : (ch + 1) * kBoxRowBuf) + tid;
            const bool more = ni < M && ne < R1;
            double gn = kInf, hn = kInf;
            if (more) {
                gn = c.G[int64_t(ni) * R1 + ne];
                if (kc > 0.0) hn = c.H[int64_t(ni) * R1 + ne];
            }
            const double *Gi = c.rowG + b, *Hi = c.rowH + b;
            const int e0 = ch * kBoxRowBuf, e1 = min(R1, e0 + kBoxRowBuf);
            for (int s = tid; s < R1; s += kWideThreads) {
                double best = ch == 0 ? kInf : nxt[s];
                int be = kBoxNone;
                const int eh = min(e1, s + 1);
                for (int e = e0; e < eh; ++e) {
                    if (kc > 0.0 && !(Hi[e - e0] <= T)) continue;
                    const double v = cur[s - e] + Gi[e - e0];
                    if (v < best) {
                        best = v;
                        be = e;
                    }
                }
                nxt[s] = best;
                if constexpr (kArg)
                    if (ch == 0 || be != kBoxNone) ai[s] = uint16_t(be);
            }
            b = kBoxRowBuf - b;
            if (more) {
                c.rowG[b + tid] = gn;
                if (kc > 0.0) c.rowH[b + tid] = hn;
            }
            __syncthreads();
        }
        double *t = cur;
        cur = nxt;
        nxt = t;
    }
    const double fin = cur[R1 - 1];
    __syncthreads();  // the next pass rewrites the planes
    return fin;
}

struct BoxesWideArgs {
    const int32_t *w_min, *w_max, *n_min, *n_max;  // halda_boxes: [n_box * dev_off[n_fleets]]; any may be NULL
    int n_box;
};

// One (box, fleet) item. A fleet of at most 64 devices lies lane = device in EVERY wave (fleet_offsets_regs's
// constants; wave 0 builds its rows and prices its plans as frontier_item does); a wider one lies thread = device:
// wave q builds the rows of devices 64 q .. 64 q + 63 from its lanes' records, and wave 0 prices a plan in
// eval_plan_wide's order (lane-strided partial sums in ascending device order, the wave sum, fleet_offsets_tree's
// constants). Either way the raw obj of an OPTIMAL (item, k) is halda_eval_plans' of the returned (k, w, n).
// Every record is a box record: without n arrays its n box is [0, INT32_MAX], the bound record's interval.
__device__ inline void boxes_wide_item(const SweepArgs &A, const BoxesWideArgs &J, int it, int b, int f, int64_t nd,
                                       const BoxesWideCtx &c, WideRed &R, int tid) {
    const int lane = tid & 63, q = tid >> 6;
    const Wave sg(lane);
    const FleetOut &O = A.out;
    const int64_t d0 = A.uM > 0 ? sload_i64(A.F.dev_off) + int64_t(f) * A.uM : sload_i64(A.F.dev_off + f);
    const int M = A.uM > 0 ? A.uM : int(sload_i64(A.F.dev_off + f + 1) - d0);
    const bool narrow = M <= 64;
    const int dev = narrow ? lane : tid;  // the device whose record the thread holds
    const bool act = dev < M;
    const bool own = tid < M;             // ... and whose rows, sums and plan entries are this thread's
    const int64_t off = int64_t(b) * nd;  // the box's plane of every bound array and of w / n
    const int64_t g0 = d0 + (act ? dev : 0);
    const int wmn = J.w_min ? J.w_min[off + g0] : 0;
    const int wmx = J.w_max ? J.w_max[off + g0] : 0x7fffffff;
    const int nmn = J.n_min ? J.n_min[off + g0] : 0;
    const int nmx = J.n_max ? J.n_max[off + g0] : 0x7fffffff;
    const DevFields mf = load_fields(A.F, g0);
    BoxRec me = {};
    int bad = 0;
    static_cast<FieldRec &>(me) = field_rec(A.Mo, mf, bad);
    double tsum = 0.0, xsum = 0.0, kappa = 0.0;
    if (narrow) fleet_offsets_regs<Wave, false>(A.Mo, mf, M, sg, tsum, xsum, kappa);
    else fleet_offsets_tree(A.Mo, A.F, d0, M, lane, tsum, xsum, kappa);
    bad = R.any(sg, own && bad != 0) ? 1 : 0;
    // the folded bounds (box_fold's, over the workgroup): lo = max(1, w_min, nlo); the three bound tests are
    // formed once for every k of the call, as bounded_fleet forms them
    me.nlo = min(max(0, nmn), kBoundCap);
    me.nhi = nmx;
    const int lo = max(min(max(1, wmn), kBoundCap), me.nlo);
    const bool cross = R.any(sg, own && (lo > wmx || me.nlo > min(me.gpu ? 0x7fffffff : 0, nmx)));
    const int64_t sumlo = R.sum(sg, own ? lo : 0);
    const int64_t sumhi = R.sum(sg, own ? min(max(wmx, 0), kBoundCap) : 0);
    if (own && tid < c.mmax) c.wlo[tid] = lo;
    double best = kInf;
    int best_k = 0;
    for (int j = 0; j < A.n_k; ++j) {
        const int k = A.ks[j], W = A.Ws[j];
        const int64_t inst = int64_t(it) * A.n_k + j;
        const double kc = double(k - 1);
        const int64_t Rr = int64_t(W) - sumlo;
        int st = HALDA_STATUS_OPTIMAL;
        if (!(W < 1000000)) st = HALDA_STATUS_UNSUPPORTED;
        else if (sumlo > W) st = HALDA_STATUS_INFEASIBLE;  // sum lb(w) > W (without bounds: M > W)
        else if (bad) st = HALDA_STATUS_UNSUPPORTED;
        else if (cross || sumhi < W) st = HALDA_STATUS_INFEASIBLE;
        else if (Rr + 1 > c.S || M > c.mmax) st = HALDA_STATUS_TOO_LARGE;  // a guard: the host sizes the slice
        double obj = kInf;
        if (st == HALDA_STATUS_OPTIMAL) {
            const int R1 = int(Rr) + 1;
            opaque_rec(me);
            me.W = W;
            me.wlo = lo;
            me.whi = min(W, wmx);
            __syncthreads();  // the previous k's plan row has been read
            {
                // the wave's devices as one table_pass of their own: rows at the devices' places in the workspace
                Inst I = {};
                I.inst = int(inst);
                I.M = narrow ? (q == 0 ? M : 0) : min(max(M - 64 * q, 0), 64);
                I.W = W;
                I.Wd = double(W);
                I.kc = kc;
                I.iC = 7 * M;
                I.R1 = R1;
                I.RS = R1;
                WaveCtx w = {};
                w.G = c.G + int64_t(64 * q) * R1;
                w.H = kc > 0.0 ? c.H + int64_t(64 * q) * R1 : nullptr;
                if (I.M > 0) table_pass<64>(bound_src(&me), w, I, lane);
            }
            __syncthreads();
            bool feas;
            if (kc == 0.0) {
                feas = boxes_wide_dp<true>(c, M, R1, 0.0, kInf, tid) < kInf;
            } else {
                // §2's exact scan, a DP pass per candidate T: the distinct finite H values in ascending order from
                // max_i min_e H_i[e]; closed once (k - 1) T + S_inf >= best. No convexity is assumed.
                const double sinf = boxes_wide_dp<false>(c, M, R1, 0.0, kInf, tid);
                double hmin = kInf;
                if (own)
                    for (int e = 0; e < R1; ++e) hmin = fmin(hmin, c.H[int64_t(tid) * R1 + e]);
                double T = R.max_f64(sg, own ? hmin : 0.0);
                double bv = kInf, bT = kInf;
                while (T < kInf && sinf < kInf) {
                    if (kc * T + sinf >= bv) break;
                    const double v = kc * T + boxes_wide_dp<false>(c, M, R1, kc, T, tid);
                    if (v < bv) {  // strict: the earliest T wins
                        bv = v;
                        bT = T;
                    }
                    double nx = kInf;  // the next distinct finite H above T
                    for (int t = tid; t < M * R1; t += kWideThreads) {
                        const double h = c.H[t];
                        if (h > T) nx = fmin(nx, h);
                    }
                    T = R.min_f64(sg, nx);
                }
                feas = bv < kInf;
                if (feas) boxes_wide_dp<true>(c, M, R1, kc, bT, tid);  // the winning T once more, with arg-mins
            }
            if (feas && tid == 0) {
                int s = R1 - 1;
                for (int i = M - 1; i >= 0; --i) {
                    const int e = min(int(c.arg[int64_t(i) * R1 + s]), s);  // (a reached state's entry is <= s)
                    c.plan[i] = uint16_t(e);
                    s -= e;
                }
            }
            __syncthreads();
            if (feas && q == 0) {
                double gsum, hmax;
                if (narrow) {
                    double gd = 0.0, H = 0.0;
                    if (act) {
                        const int wl = lo + c.plan[lane];
                        double Pc, Qc;
                        int n = 0, sl[4] = {0, 0, 0, 0};
                        split_full(me, wl, gd, n, sl);
                        dev_cycle(me, wl, n, sl, Pc, Qc);
                        H = fmax(0.0, Qc >= Pc ? 0.5 * (Pc + Qc) : Pc);
                        c.nplan[lane] = n;
                    }
                    hmax = sg.max_f64(act ? H : 0.0);
                    gsum = sg.sum_f64(act ? gd : 0.0);
                } else {
                    double gs = 0.0, hm = 0.0;
                    for (int i = lane; i < M; i += 64) {
                        BoxRec ri = {};
                        int bi = 0;
                        static_cast<FieldRec &>(ri) = field_rec(A.Mo, load_fields(A.F, d0 + i), bi);
                        ri.W = W;
                        ri.wlo = c.wlo[i];
                        ri.whi = W;
                        ri.nlo = min(max(0, J.n_min ? J.n_min[off + d0 + i] : 0), kBoundCap);
                        ri.nhi = J.n_max ? J.n_max[off + d0 + i] : 0x7fffffff;
                        const int wl = ri.wlo + c.plan[i];
                        double gd = 0.0, Pc, Qc;
                        int n = 0, sl[4] = {0, 0, 0, 0};
                        split_full(ri, wl, gd, n, sl);
                        dev_cycle(ri, wl, n, sl, Pc, Qc);
                        c.nplan[i] = n;
                        gs += gd;
                        hm = fmax(hm, fmax(0.0, Qc >= Pc ? 0.5 * (Pc + Qc) : Pc));
                    }
                    hmax = sg.max_f64(hm);
                    gsum = sg.sum_f64(gs);
                }
                double o = gsum + kc * hmax;
                o = o + tsum;
                o = o + xsum;
                o = o + kappa;
                if (lane == 0) c.pick[j] = o;
            }
            __syncthreads();
            if (feas) obj = c.pick[j];
            else st = HALDA_STATUS_INFEASIBLE;
            if (obj < best) {  // ascending k, strict: the smallest k wins
                best = obj;
                best_k = k;
                if (own) {
                    O.w[off + d0 + tid] = lo + c.plan[tid];
                    O.n[off + d0 + tid] = c.nplan[tid];
                }
            }
        }
        if (tid == 0) {
            if (A.outs & kOutObk) O.obj_by_k[inst] = obj;
            if (A.outs & kOutSt) O.status[inst] = st;
        }
    }
    if (tid == 0) {
        O.best_k[it] = best_k;
        O.obj_value[it] = best;
    }
    if (best_k == 0 && own) {
        O.w[off + d0 + tid] = 0;
        O.n[off + d0 + tid] = 0;
    }
    __syncthreads();  // the LDS and the workspace slice are rewritten by the workgroup's next item
}

// One 256-thread workgroup per (box, fleet) item on a persistent grid (workgroup g takes items g, g + grid, ...;
// item it is box it / nf, fleet it % nf), its LDS and its workspace slice (A.gtab + g A.gstride) laid out by
// boxes_wide_slice of the launch's shape (A.mmax devices, A.r1max = max R + 1). Every barrier is reached by every
// thread; no spin-wait, no atomics, nothing shared between workgroups.
__global__ __launch_bounds__(kWideThreads) void halda_sweep_boxes_wide_kernel(SweepArgs A, BoxesWideArgs Bs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const BoxesWideSlice sl = boxes_wide_slice(A.mmax, A.r1max - 1, A.ks[A.n_k - 1] > 1);
    const BoxesWideCtx c = boxes_wide_ctx(smem, A.gtab + int64_t(blockIdx.x) * A.gstride, sl, A.mmax);
    WideRed R = {smem + sl.red, 0, tid >> 6, tid & 63};
    const int nf = A.F.n_fleets;
    const int64_t nd = sload_i64(A.F.dev_off + nf), items = int64_t(Bs.n_box) * nf;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int b = int(it / nf), f = int(it - int64_t(b) * nf);
        boxes_wide_item(A, Bs, int(it), b, f, nd, c, R, tid);
    }
}
