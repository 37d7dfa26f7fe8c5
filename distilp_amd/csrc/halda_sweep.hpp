// halda_sweep.hpp -- the whole k-sweep (halda_solve_fleets): the GPU lowering, the fused sweep kernels
// (register, pipelined, table, segment, k-slot) and the CSR path's pick kernel.
// Part of libhalda's single translation unit: included by halda.hip inside its anonymous namespace
// (after halda_solve.hpp); not a standalone header.
#pragma once
// ---------------------------------------------------------------- GPU lowering
// halda_lower_kernel: one wave per fleet, lane = device, writes the fleet's
// fixed-k MILPs for every k-candidate into the halda_batch layout with fixed
// per-fleet strides (solve kernels read them unchanged). Restates the host
// lowering (distilp_amd/solver/lower.py, itself the reference's
// solve_fixed_k_milp, halda_p_solver.py:59-338, with dense_common.py:25-230):
// same row order, same zero-dropping, same FP operation order -> the same CSR
// and vectors bit for bit. An instance with W = L / k < M (every device needs a
// layer: bound-infeasible, 8 of the 9 k at M = 64, L = 80) gets only what the
// screen settles it from: header, w bounds, c[C] and the equality row's bounds.
struct LowerDims {
    int mmax, n_k;
    int64_t cols, rows, nnz;  // strides per instance (cols, rows) and per fleet (nnz)
};

__host__ __device__ inline LowerDims lower_dims(int mmax, int n_k) {
    LowerDims d;
    d.mmax = mmax;
    d.n_k = n_k;
    d.cols = 7 * int64_t(mmax) + 1;
    d.rows = 6 * int64_t(mmax) + 1;   // link M, capacity <= M, VRAM <= 2M, cycle 2M, equality 1
    d.nnz = 26 * int64_t(mmax);       // 2M + 3M + 4M + 16M + M
    return d;
}

// Exclusive prefix sum over the wave (all lanes active); total in *tot.
__device__ inline int wave_excl_scan(int v, int lane, int *tot) {
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    *tot = __shfl(x, 63);
    return x - v;
}

// sum_f_over_s (dense_common.py:49-75) for a key/quantisation known present or absent.
__device__ inline double f_over_s(bool present, double f, double s) {
    return present ? (s > 0.0 ? 0.0 + f / s : 0.0) : 0.0;
}

// Per-device coefficients of the fixed-k MILP (dense_common.py:25-126 and the penalties of
// halda_p_solver.py:195-224) in the reference's operation order; shared by the lowering kernel
// (CSR out) and the sweep kernel (records straight into registers), so both see the same bits.
struct DevCoef {
    double alpha, b, p_bp, p_b, p_v, cst, bcio, xi;
};

// One device's table entry in registers: every field loaded unconditionally (one memory round
// trip for all of them), the coefficients computed from the registers.
struct DevFields {
    double scpu, sgpu, Tc, Tg, tkc, tkg, r2v, v2r, tcomm, sdisk;
    double ram, ccpu, cgpu, cuda, metal, swap;  // byte counts: integers below 2^53, so the integer sums and
                                                // differences of the reference are exact in double
    int cls, flags;
};

__device__ inline DevFields load_fields(const halda_fleets &F, int64_t g) {
    DevFields f;
    f.scpu = F.scpu_b1[g]; f.sgpu = F.sgpu_b1[g]; f.Tc = F.T_cpu[g]; f.Tg = F.T_gpu[g];
    f.tkc = F.t_kvcpy_cpu[g]; f.tkg = F.t_kvcpy_gpu[g]; f.r2v = F.t_ram2vram[g]; f.v2r = F.t_vram2ram[g];
    f.tcomm = F.t_comm[g]; f.sdisk = F.s_disk[g];
    f.ram = F.d_avail_ram[g]; f.ccpu = F.c_cpu[g]; f.cgpu = F.c_gpu[g]; f.cuda = F.d_avail_cuda[g];
    f.metal = F.d_avail_metal[g]; f.swap = F.swap[g];
    f.cls = F.os_class[g];
    f.flags = F.flags[g];
    return f;
}

// load_fields with a 32-bit device index (the table's arrays below 4 GiB: the host checks): each load is
// the array's base in SGPRs plus one shared 32-bit byte offset, no per-field 64-bit address arithmetic
// (the steps kernel: 864 -> 845 VALU per C3 item).
template <class T>
__device__ inline T at32(const T *p, uint32_t boff) {
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(p) + boff);
}
__device__ inline DevFields load_fields32(const halda_fleets &F, uint32_t g) {
    const uint32_t o8 = g * 8u;
    DevFields f;
    f.scpu = at32(F.scpu_b1, o8); f.sgpu = at32(F.sgpu_b1, o8); f.Tc = at32(F.T_cpu, o8); f.Tg = at32(F.T_gpu, o8);
    f.tkc = at32(F.t_kvcpy_cpu, o8); f.tkg = at32(F.t_kvcpy_gpu, o8); f.r2v = at32(F.t_ram2vram, o8);
    f.v2r = at32(F.t_vram2ram, o8); f.tcomm = at32(F.t_comm, o8); f.sdisk = at32(F.s_disk, o8);
    f.ram = at32(F.d_avail_ram, o8); f.ccpu = at32(F.c_cpu, o8); f.cgpu = at32(F.c_gpu, o8);
    f.cuda = at32(F.d_avail_cuda, o8); f.metal = at32(F.d_avail_metal, o8); f.swap = at32(F.swap, o8);
    f.cls = at32(F.os_class, g);
    f.flags = at32(F.flags, g);
    return f;
}

// The model as the sweep kernels see it: halda_model plus the uniform quotient (b_in / V) + b_out
// formed once on the host (the same IEEE double operations, -ffp-contract=off: the same bits) instead
// of by every wave.
struct SweepModel : halda_model {
    double bvo;  // (b_in / V) + b_out
};

__host__ __device__ inline double model_bvo(const halda_model &Mo) { return (Mo.b_in / Mo.V) + Mo.b_out; }

__device__ inline DevCoef dev_coef(const halda_model &Mo, const DevFields &F, double bvo) {
    DevCoef o;
    const double bp = Mo.b_prime;
    const int fl = F.flags;
    const int cls = F.cls;
    const double Tc = F.Tc, tkc = F.tkc, tkg = F.tkg;
    const double cpu = f_over_s(Mo.has_f_q && (fl & HALDA_DEV_CPU_RATE), Mo.f_q_b1, F.scpu);
    const bool hb = fl & HALDA_DEV_GPU;
    const double gpu = hb ? f_over_s(Mo.has_f_q && (fl & HALDA_DEV_GPU_RATE), Mo.f_q_b1, F.sgpu) : 0.0;
    const double tg = hb ? F.Tg : 1.0;
    o.alpha = (cpu + tkc) + (bp / Tc);
    const double beta = hb ? ((gpu - cpu) + (tkg - tkc)) + (bp / tg - bp / Tc) : 0.0;
    o.b = cls == 1 ? 0.0 : beta;
    o.xi = (F.r2v + F.v2r) * ((fl & HALDA_DEV_UMA) ? 0.0 : 1.0);
    const double head = (fl & HALDA_DEV_HEAD) ? 1.0 : 0.0;
    o.bcio = bvo * head + F.ccpu;
    const double sd = fmax(1.0, F.sdisk);
    o.p_bp = bp / sd;
    o.p_b = Mo.b_layer / sd;
    o.p_v = cls == 2 ? o.p_b : o.p_bp;
    o.cst = o.xi + F.tcomm;
    return o;
}

__device__ inline DevCoef dev_coef(const halda_model &Mo, const DevFields &F) { return dev_coef(Mo, F, model_bvo(Mo)); }

__device__ inline DevCoef dev_coef(const halda_model &Mo, const halda_fleets &F, int64_t g) {
    return dev_coef(Mo, load_fields(F, g));
}

// Right-hand sides of the capacity rows (halda_p_solver.py:227-277).
__device__ inline double rhs_ram(const DevFields &F, int set, double bcio) {
    if (set == 1) return F.ram - bcio;
    if (set == 2) return F.metal - bcio - F.cgpu;
    return (F.ram + F.swap) - bcio;  // the reference's integer sum, exact
}
__device__ inline double rhs_cuda(const DevFields &F) { return F.cuda - F.cgpu; }
__device__ inline double rhs_metal(const halda_model &Mo, const DevFields &F) {
    const double head = (F.flags & HALDA_DEV_HEAD) ? 1.0 : 0.0;
    return F.metal - F.cgpu - Mo.b_out * head;
}
__device__ inline double rhs_ram(const halda_fleets &F, int64_t g, int set, double bcio) {
    return rhs_ram(load_fields(F, g), set, bcio);
}
__device__ inline double rhs_cuda(const halda_fleets &F, int64_t g) { return rhs_cuda(load_fields(F, g)); }
__device__ inline double rhs_metal(const halda_model &Mo, const halda_fleets &F, int64_t g) {
    return rhs_metal(Mo, load_fields(F, g));
}

// Objective constants of one fleet (lane-parallel loads, the reference's sequential sums over
// readlane): sum t_comm and sum xi in device order, kappa (dense_common.py:211-230) with its
// M1 part before its M3 part (:226). Uniform on every lane.
__device__ inline void fleet_offsets(const halda_model &Mo, const halda_fleets &F, int64_t d0, int M, int lane,
                                     double &tsum, double &xsum, double &kappa) {
    tsum = 0.0;
    xsum = 0.0;
    double tail1 = 0.0;
    int hi = -1;
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int i = min(i0 + lane, M - 1);
        const int64_t g = d0 + i;
        const double tc = F.t_comm[g];
        const double xv = (F.t_ram2vram[g] + F.t_vram2ram[g]) * ((F.flags[g] & HALDA_DEV_UMA) ? 0.0 : 1.0);
        const int cls = F.os_class[g];
        const double tl = ((F.c_cpu[g] - F.d_avail_ram[g]) - F.swap[g]) / F.s_disk[g];
        const uint64_t heads = __ballot(i0 + lane < M && (F.flags[g] & HALDA_DEV_HEAD));
        if (hi < 0 && heads) hi = i0 + __builtin_ctzll(heads);
        const int n = min(64, M - i0);
        for (int q = 0; q < n; ++q) {
            tsum += bcast(tc, q);
            xsum += bcast(xv, q);
            const int cq = bcast(cls, q);
            if (cq == 1) tail1 += bcast(tl, q);
        }
    }
    double tail = tail1;
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int i = min(i0 + lane, M - 1);
        const int64_t g = d0 + i;
        const int cls = F.os_class[g];
        const double tl = ((F.c_cpu[g] - F.d_avail_ram[g]) - F.swap[g]) / F.s_disk[g];
        const int n = min(64, M - i0);
        for (int q = 0; q < n; ++q)
            if (bcast(cls, q) == 3) tail += bcast(tl, q);
    }
    const int64_t h = d0 + (hi < 0 ? 0 : hi);
    double total = f_over_s(Mo.has_f_out && (F.flags[h] & HALDA_DEV_CPU_RATE), Mo.f_out_b1, F.scpu_b1[h]);
    total += (Mo.b_in / Mo.V + Mo.b_out) / F.T_cpu[h];
    total += Mo.b_in / (Mo.V * F.s_disk[h]);
    total += Mo.b_out / F.s_disk[h];
    kappa = total + tail;
}

struct LowerOut {
    halda_batch b;         // arrays written (device pointers, const-cast by the kernel)
    int32_t *n_cols, *n_rows, *row_ptr, *col_idx;
    int64_t *csr_off, *col_off, *row_off;
    double *val, *c, *col_lb, *col_ub, *row_lb, *row_ub, *offs;  // offs[f]: t_comm sum, xi sum, kappa
    uint8_t *integrality;
};

__global__ __launch_bounds__(64) void halda_lower_kernel(halda_model Mo, halda_fleets F, const int32_t *ks, int n_k,
                                                         LowerDims D, LowerOut O) {
    const int lane = threadIdx.x;
    const int f = blockIdx.x;
    if (f >= F.n_fleets) return;
    const int64_t d0 = F.dev_off[f];
    const int M = int(F.dev_off[f + 1] - d0);
    const int64_t nnz0 = int64_t(f) * D.nnz;       // this fleet's CSR entries
    const int64_t rp0 = int64_t(f) * (D.rows + 1);  // this fleet's row_ptr segment
    const double bp = Mo.b_prime;
    const int iC = 7 * M;
    int rows = 0;
    int64_t nnz = 0;
    // per-block row emission: lane i emits up to 2 rows for device i (chunks of 64). Two passes of the
    // row function: count the nonzeros, scan, then write the entries straight to the CSR (no private
    // arrays: dynamically indexed ones would live in scratch).
    auto emit = [&](auto &&row_fn) {
        for (int i0 = 0; i0 < M; i0 += 64) {
            const int i = i0 + lane;
            const bool act = i < M;
            int c0 = 0, c1 = 0;
            double r0 = 0.0, r1 = 0.0;
            const int nr = act ? row_fn(i, false, c0, c1, r0, r1, int64_t(0), int64_t(0)) : 0;
            int rtot = 0, ntot = 0;
            const int rbase = wave_excl_scan(nr, lane, &rtot);
            const int nbase = wave_excl_scan(c0 + c1, lane, &ntot);
            if (nr > 0) {
                const int64_t e0 = nnz0 + nnz + nbase, e1 = e0 + c0;
                int w0 = 0, w1 = 0;
                row_fn(i, true, w0, w1, r0, r1, e0, e1);
                const int r = rows + rbase;
                O.row_ptr[rp0 + r] = int32_t(e0);
                if (nr > 1) O.row_ptr[rp0 + r + 1] = int32_t(e1);
                for (int j = 0; j < n_k; ++j) {
                    if (Mo.L / ks[j] < M) continue;  // bound-infeasible: the screen reads only the eq row
                    const int64_t ro = (int64_t(f) * n_k + j) * D.rows;
                    O.row_lb[ro + r] = -kInf;
                    O.row_ub[ro + r] = r0;
                    if (nr > 1) {
                        O.row_lb[ro + r + 1] = -kInf;
                        O.row_ub[ro + r + 1] = r1;
                    }
                }
            }
            rows += rtot;
            nnz += ntot;
        }
    };
    // one (col, val) of a row when val != 0 (scipy builds its CSC from the dense rows): counted, or
    // written at e + n when wr
    auto put = [&](bool wr, int64_t e, int &n, int col, double v) {
        if (v != 0.0) {
            if (wr) {
                O.col_idx[e + n] = col;
                O.val[e + n] = v;
            }
            ++n;
        }
    };
    // ---- per-device coefficients (lower._device_arrays order); lane i's own device is computed once
    DevCoef mine = {};
    if (lane < M) mine = dev_coef(Mo, F, d0 + lane);
    auto coeff = [&](int i, double &alpha, double &b, double &p_bp, double &p_b, double &p_v, double &cst,
                     double &bcio, double &xi) {
        const DevCoef c = i == lane ? mine : dev_coef(Mo, F, d0 + i);
        alpha = c.alpha; b = c.b; p_bp = c.p_bp; p_b = c.p_b; p_v = c.p_v; cst = c.cst; bcio = c.bcio; xi = c.xi;
    };
    // 1. link rows n_i - w_i <= 0
    emit([&](int i, bool wr, int &c0, int &c1, double &r0, double &r1, int64_t e0, int64_t e1) {
        (void)c1; (void)r1; (void)e1;
        put(wr, e0, c0, i, -1.0);
        put(wr, e0, c0, M + i, 1.0);
        r0 = 0.0;
        return 1;
    });
    // 2-4. RAM / Metal capacity rows by set
    for (int set = 1; set <= 3; ++set) {
        emit([&](int i, bool wr, int &c0, int &c1, double &r0, double &r1, int64_t e0, int64_t e1) {
            (void)c1; (void)r1; (void)e1;
            const int64_t g = d0 + i;
            if (F.os_class[g] != set) return 0;
            if (set == 2 && !(F.flags[g] & HALDA_DEV_METAL_AVAIL)) return 0;
            double alpha, b, p_bp, p_b, p_v, cst, bcio, xi;
            coeff(i, alpha, b, p_bp, p_b, p_v, cst, bcio, xi);
            put(wr, e0, c0, i, bp);
            if (set == 3) put(wr, e0, c0, M + i, -bp);
            put(wr, e0, c0, (1 + set) * M + i, -bp);
            r0 = rhs_ram(F, g, set, bcio);
            return 1;
        });
    }
    // 5. VRAM rows: per device the CUDA row, then the Metal row
    emit([&](int i, bool wr, int &c0, int &c1, double &r0, double &r1, int64_t e0, int64_t e1) {
        const int64_t g = d0 + i;
        const uint8_t fl = F.flags[g];
        const bool cu = fl & HALDA_DEV_CUDA_OK, me = fl & HALDA_DEV_METAL_OK;
        const double rc = rhs_cuda(F, g);
        const double rm = rhs_metal(Mo, F, g);
        if (cu) {
            put(wr, e0, c0, M + i, bp);
            put(wr, e0, c0, 5 * M + i, -bp);
            r0 = rc;
        }
        if (me) {
            int &cm = cu ? c1 : c0;
            const int64_t em = cu ? e1 : e0;
            put(wr, em, cm, M + i, bp);
            put(wr, em, cm, 5 * M + i, -bp);
            (cu ? r1 : r0) = rm;
        }
        return int(cu) + int(me);
    });
    // 6. cycle rows busy + z - C <= -const ; busy + F - z - C <= -const
    emit([&](int i, bool wr, int &c0, int &c1, double &r0, double &r1, int64_t e0, int64_t e1) {
        double alpha, b, p_bp, p_b, p_v, cst, bcio, xi;
        coeff(i, alpha, b, p_bp, p_b, p_v, cst, bcio, xi);
        put(wr, e0, c0, i, alpha);
        put(wr, e1, c1, i, alpha + p_bp);
        put(wr, e0, c0, M + i, b);
        put(wr, e1, c1, M + i, b);
        put(wr, e0, c0, 2 * M + i, p_bp);
        put(wr, e1, c1, 2 * M + i, p_bp);
        put(wr, e0, c0, 3 * M + i, p_b);
        put(wr, e1, c1, 3 * M + i, p_b);
        put(wr, e0, c0, 4 * M + i, p_bp);
        put(wr, e1, c1, 4 * M + i, p_bp);
        put(wr, e0, c0, 5 * M + i, p_v);
        put(wr, e1, c1, 5 * M + i, p_v);
        put(wr, e0, c0, 6 * M + i, 1.0);
        put(wr, e1, c1, 6 * M + i, -1.0);
        put(wr, e0, c0, iC, -1.0);
        put(wr, e1, c1, iC, -1.0);
        r0 = r1 = -cst;
        return 2;
    });
    // 7. equality row sum_i w_i = W (row bounds per k below)
    {
        const int r = rows;
        O.row_ptr[rp0 + r] = int32_t(nnz0 + nnz);
        for (int i = lane; i < M; i += 64) {
            O.col_idx[nnz0 + nnz + i] = i;
            O.val[nnz0 + nnz + i] = 1.0;
        }
        nnz += M;
        rows += 1;
        if (lane == 0) O.row_ptr[rp0 + rows] = int32_t(nnz0 + nnz);
    }
    // ---- per-instance vectors (lane = device) and headers
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int i = i0 + lane;
        if (i >= M) continue;
        const int64_t g = d0 + i;
        const uint8_t fl = F.flags[g];
        const int cls = F.os_class[g];
        double alpha, b, p_bp, p_b, p_v, cst, bcio, xi;
        coeff(i, alpha, b, p_bp, p_b, p_v, cst, bcio, xi);
        const double busy[6] = {alpha, b, p_bp, p_b, p_bp, p_v};
        const double gpu = (fl & (HALDA_DEV_CUDA_OK | HALDA_DEV_METAL_OK)) ? 1.0 : 0.0;
        const double scale[6] = {1.0, gpu, cls == 1 ? 1.0 : 0.0, cls == 2 ? 1.0 : 0.0, cls == 3 ? 1.0 : 0.0, gpu};
        for (int j = 0; j < n_k; ++j) {
            const double W = double(Mo.L / ks[j]);
            const int64_t co = (int64_t(f) * n_k + j) * D.cols;
            if (Mo.L / ks[j] < M) {
                // W < M = sum lb(w): the screen settles it from the w bounds (and c[C], the eq row)
                O.col_lb[co + i] = 1.0;
                O.col_ub[co + i] = W;
                continue;
            }
#pragma unroll
            for (int blk = 0; blk < 6; ++blk) {
                O.c[co + blk * M + i] = busy[blk];
                O.col_lb[co + blk * M + i] = blk == 0 ? 1.0 : 0.0;
                O.col_ub[co + blk * M + i] = scale[blk] * W;
                O.integrality[co + blk * M + i] = 1;
            }
            O.c[co + 6 * M + i] = 0.0;
            O.col_lb[co + 6 * M + i] = 0.0;
            O.col_ub[co + 6 * M + i] = kInf;
            O.integrality[co + 6 * M + i] = 0;
        }
    }
    for (int j = lane; j < n_k; j += 64) {
        const int64_t inst = int64_t(f) * n_k + j;
        const int64_t co = inst * D.cols, ro = inst * D.rows;
        const double W = double(Mo.L / ks[j]);
        O.c[co + iC] = double(ks[j] - 1);
        O.col_lb[co + iC] = 0.0;
        O.col_ub[co + iC] = kInf;
        O.integrality[co + iC] = 0;
        O.row_lb[ro + rows - 1] = W;
        O.row_ub[ro + rows - 1] = W;
        O.n_cols[inst] = 7 * M + 1;
        O.n_rows[inst] = rows;
        O.csr_off[inst] = rp0;
        O.col_off[inst] = co;
        O.row_off[inst] = ro;
    }
    // ---- objective offsets: sum t_comm and sum xi in device order, kappa (dense_common.py:211-230)
    double tsum, xsum, kappa;
    fleet_offsets(Mo, F, d0, M, lane, tsum, xsum, kappa);
    if (lane == 0) {
        O.offs[3 * f + 0] = tsum;
        O.offs[3 * f + 1] = xsum;
        O.offs[3 * f + 2] = kappa;
    }
}

// ---------------------------------------------------------------- fused k-sweep
// halda_sweep_kernel: the whole `halda_solve` k-sweep of a fleet (halda_p_solver.py:369-436) in
// one wave, from the fleet's device-field table, without materialising the MILPs. For every
// k-candidate the wave builds, per device, exactly the record that decoding the lowered CSR
// yields (load_dev of decode_cap_row / decode_cycle_row output, with the same rejections),
// straight from the coefficients the lowering kernel writes into the CSR (dev_coef / rhs_* are
// shared, so the values are the same bits); then settles bound-infeasible k (L / k < M), solves
// k = 1 by the register greedy of the k = 1 fast path and the rest (k > 1, fleets wider than
// 64 devices, fast-path fallbacks) by the general kernel's tables + DP / threshold scan, and keeps
// the best k by the reference's rule (ascending k, strict "<" on obj_value, :407) in registers.
// obj_value = c.x + sum t_comm + sum xi + kappa is formed in a fixed order (per-device costs
// summed by a wave reduction, + (k - 1) C, + the fleet constants).
//
// kTables = false: no LDS; a fleet that needs a table is flagged (fflag[f] = 1, hb_flag = launch)
// and left to the next launch. kTables = true: tables in the LDS slice (kGlobal = false) or in a
// per-wave global slice (kGlobal = true); want = 1 selects the flagged fleets only (gated on the
// hand-back flag), want = 0 every fleet.

// FieldRec (the compact device record) and its specialised solve primitives: halda_solve.hpp.

__device__ inline FieldRec field_rec(const SweepModel &Mo, const DevFields &F, int &bad) {
    FieldRec r;
    const DevCoef c = dev_coef(Mo, F, Mo.bvo);
    const double bp = Mo.b_prime;
    const int fl = F.flags;
    r.alpha = c.alpha; r.b = c.b; r.p_bp = c.p_bp; r.p_b = c.p_b; r.cst = c.cst;
    r.cls = F.cls;
    r.gpu = (fl & (HALDA_DEV_CUDA_OK | HALDA_DEV_METAL_OK)) ? 1 : 0;
    r.W = 0;
    r.Kset = r.Kvram = kNoRow;
    bad = !(fabs(c.cst) < 1e300);  // cycle-row rhs
    bad |= !(c.p_bp >= 0.0) || !(c.p_b >= 0.0) || !(r.cls == 2 ? c.p_b >= 0.0 : c.p_bp >= 0.0);  // slack prices
    // capacity rows b' u w + b' v n - b' s <= rhs -> s >= u w + v n + ceil(-rhs / b' - eps)
    auto K = [&](double rhs, int &dst) {
        if (!(bp > 0.0) || !(fabs(rhs) < 1e300)) {
            bad = 1;
            return;
        }
        const double kk = ceil(-rhs / bp - kSlackEps);
        if (!(fabs(kk) < 1e8)) {
            bad = 1;
            return;
        }
        dst = max(dst, int(kk));
    };
    if (r.cls == 1 || r.cls == 3 || (fl & HALDA_DEV_METAL_AVAIL)) K(rhs_ram(F, r.cls, c.bcio), r.Kset);
    // VRAM rows: CUDA or Metal (one division for either; both rows only on a device with both)
    const bool cu = fl & HALDA_DEV_CUDA_OK, mt = fl & HALDA_DEV_METAL_OK;
    if (cu && mt) {
        K(rhs_cuda(F), r.Kvram);
        K(rhs_metal(Mo, F), r.Kvram);
    } else if (cu || mt) {
        K(cu ? rhs_cuda(F) : rhs_metal(Mo, F), r.Kvram);
    }
    return r;
}

// Device records of a fleet straight from its table (the sweep's table path).
// Device records of a fleet for the sweep's table path: for M <= 64 lane i already holds device
// i's record (me), which other lanes fetch by shuffle; wider fleets rebuild it from the table.
// load() runs on every lane (uniform control flow: the shuffles read every lane's registers).
struct FieldSrc {
    using Rec = FieldRec;
    const SweepModel *Mo;
    const halda_fleets *F;
    const FieldRec *me;  // lane's own record (M <= lanes per problem), or nullptr
    int64_t d0;
    int W;
    int base;            // first lane of the problem's lane group
    __device__ inline void load(FieldRec &r, const WaveCtx &, int i) const {
        if (me) {
            r = me->shfl(base + i);
        } else {
            int bad = 0;
            r = field_rec(*Mo, load_fields(*F, d0 + i), bad);
        }
        r.W = W;
    }
};

// Objective constants of a fleet for the sweep's own obj_value (a fixed tree order: wave
// reductions): sum t_comm, sum xi, kappa with the head's terms (dense_common.py:211-230). For
// M <= 64 lane i passes device i's fields (in registers) and the head's come by readlane.
__device__ inline double tail_term(const DevFields &f) {
    return f.cls != 2 ? ((f.ccpu - f.ram) - f.swap) / f.sdisk : 0.0;
}
__device__ inline double xi_term(const DevFields &f) { return (f.r2v + f.v2r) * ((f.flags & HALDA_DEV_UMA) ? 0.0 : 1.0); }

__device__ inline double kappa_head(const halda_model &Mo, int flags, double scpu, double Tc, double sdisk) {
    double total = f_over_s(Mo.has_f_out && (flags & HALDA_DEV_CPU_RATE), Mo.f_out_b1, scpu);
    total += (Mo.b_in / Mo.V + Mo.b_out) / Tc;
    total += Mo.b_in / (Mo.V * sdisk);
    total += Mo.b_out / sdisk;
    return total;
}

template <class SG, bool kLds = false>
__device__ inline void fleet_offsets_regs(const SweepModel &Mo, const DevFields &mf, int M, const SG &sg, double &tsum,
                                          double &xsum, double &kappa) {
    const bool act = sg.sl < M;
    // one wave sum for the three per-device constants of obj_value (t_comm, xi and kappa's tail term,
    // added per device in that order): tsum carries all of it, xsum is 0 and kappa its head terms;
    // obj_value's constants are summed in this fixed order (the host recomputes the reference's own
    // order for halda_solve)
    tsum = sg.sum_f64(act ? (mf.tcomm + xi_term(mf)) + tail_term(mf) : 0.0);
    xsum = 0.0;
    int hi = sg.lowest(act && (mf.flags & HALDA_DEV_HEAD));
    if (hi >= SG::S) hi = 0;
    // kappa_head's four quotients on lanes 0..3 of the problem (one division for the four), summed in
    // its order
    const int hf = sg.bcast(mf.flags, hi);
    const double scpu = sg.bcast(mf.scpu, hi), Tc = sg.bcast(mf.Tc, hi), sdisk = sg.bcast(mf.sdisk, hi);
    const int j = sg.sl & 3;
    // the four numerators as register values: a select chain over kernel arguments is otherwise turned
    // into a per-lane vector load from the argument segment (a vector memory wait of its own)
    double n0 = Mo.f_out_b1, n1 = Mo.bvo, n2 = Mo.b_in, n3 = Mo.b_out;
    if constexpr (kLds) {  // the model read from LDS: vector registers
        asm volatile("" : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3));
    } else {
        asm volatile("" : "+s"(n0), "+s"(n1), "+s"(n2), "+s"(n3));
    }
    const double num = j == 0 ? n0 : j == 1 ? n1 : j == 2 ? n2 : n3;
    const double den = j == 0 ? scpu : j == 1 ? Tc : j == 2 ? Mo.V * sdisk : sdisk;
    const double q = num / den;
    const double q0 = sg.bcast(q, 0), q1 = sg.bcast(q, 1), q2 = sg.bcast(q, 2), q3 = sg.bcast(q, 3);
    double total = (Mo.has_f_out && (hf & HALDA_DEV_CPU_RATE)) ? (scpu > 0.0 ? 0.0 + q0 : 0.0) : 0.0;
    total += q1;
    total += q2;
    total += q3;
    kappa = total;
}

__device__ inline void fleet_offsets_tree(const halda_model &Mo, const halda_fleets &F, int64_t d0, int M, int lane,
                                          double &tsum, double &xsum, double &kappa) {
    double t = 0.0, x = 0.0, tail = 0.0;
    int hi = 0x7fffffff;
    for (int i = lane; i < M; i += 64) {
        const DevFields f = load_fields(F, d0 + i);
        t += f.tcomm;
        x += xi_term(f);
        tail += tail_term(f);
        if (f.flags & HALDA_DEV_HEAD) hi = min(hi, i);
    }
    tsum = wave_sum_f64(t);
    xsum = wave_sum_f64(x);
    tail = wave_sum_f64(tail);
    hi = wave_imin(hi);
    const int64_t h = d0 + (hi == 0x7fffffff ? 0 : hi);
    kappa = kappa_head(Mo, F.flags[h], F.scpu_b1[h], F.T_cpu[h], F.s_disk[h]) + tail;
}

// A uniform read of read-only memory through the scalar cache (s_load): the constant address space
// tells the compiler the value cannot change under the kernel (a plain global read of a uniform
// address is a vector load, a full memory round trip before the loads that depend on it).
__device__ inline int64_t sload_i64(const int64_t *p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) int64_t *>(
        reinterpret_cast<uintptr_t>(p));
}

// No instruction: the record's registers are redefined for the optimiser (stops loop-invariant
// hoisting of values derived from it).
__device__ inline void opaque_rec(FieldRec &r) {
    asm volatile("" : "+v"(r.alpha), "+v"(r.b), "+v"(r.p_bp), "+v"(r.p_b), "+v"(r.cst), "+v"(r.Kset), "+v"(r.Kvram),
                 "+v"(r.cls), "+v"(r.gpu));
}

// Kernel arguments. Everything a wave reads through the scalar cache comes first (six 64-B lines:
// the model, the table pointers, the result pointers, the counts); the k list, which lanes read
// with vector loads, last.
// halda_fleet_result without x_off (ABI 2's compact layout travels at the end of SweepArgs): the
// result pointers stay within the kernel arguments' first lines, read through the scalar cache.
struct FleetOut {
    int32_t *best_k;
    double *obj_value;
    int32_t *w, *n;
    double *obj_by_k;
    int32_t *status;
    double *x, *c;
    FleetOut() = default;
    __host__ __device__ FleetOut(const halda_fleet_result &r)
        : best_k(r.best_k), obj_value(r.obj_value), w(r.w), n(r.n), obj_by_k(r.obj_by_k), status(r.status), x(r.x),
          c(r.c) {}
};

// SweepArgs.outs: which optional outputs the call wants, in one word the waves read with the first
// kernel-argument line (testing the pointers themselves costs a dependent scalar load each)
constexpr int kOutObk = 1, kOutSt = 2, kOutX = 4, kOutC = 8, kOutXC = kOutX | kOutC, kOutXZ = 16;

struct SweepArgs {
    SweepModel Mo;
    halda_fleets F;
    int n_k;
    int uM;                        // > 0: every fleet has uM devices (dev_off[f] = dev_off[0] + f uM)
    int outs;                      // kOut* bits
    FleetOut out;
    int64_t xstride;
    uint8_t *fflag;  // per fleet: 1 = needs the table launch
    int *hb_flag;
    int launch_id;
    int want;                      // 0: every fleet, 1: flagged fleets (gated on hb_flag)
    int k1dp;                      // register sweep: 1 = every k = 1 / W = M instance by k1_dp (test path)
    int mmax, r1max, tab, tab_kc;  // table slice shape (kTables)
    unsigned char *gtab;           // kGlobal: per-wave slices
    int64_t gstride;
    const int64_t *x_off;          // halda_fleet_result.x_off (compact x / c layout) or nullptr
    int32_t ks[64];  // the k list travels in the kernel arguments (no copy)
    int32_t Ws[64];  // W = L / k per k (host integer division)
};

// The per-batch part of a sweep's arguments: the table, the results and the per-fleet hand-back flags
// (a launch's own A.F / A.out / A.fflag, or one batch of a steps launch).
// References, so that a launch's own view reads the kernel arguments where they are (no copy held in
// registers).
struct SweepBatch {
    const halda_fleets &F;
    const FleetOut &out;
    uint8_t *fflag;
};

__device__ inline SweepBatch batch_of(const SweepArgs &A) { return SweepBatch{A.F, A.out, A.fflag}; }

// Element offset of instance inst's x / c: the dense layout, or the caller's compact x_off (-1: not
// written).
__device__ inline int64_t xc_at(const SweepArgs &A, int64_t inst) {
    return A.x_off ? A.x_off[inst] : inst * A.xstride;
}

// x / c of one (fleet, k) solution (col layout [w|n|s1|s2|s3|t|z|C] with the fleet's M), written
// by the lane of each device when the caller asked for them.
__device__ inline void put_xc(const SweepArgs &A, const FleetOut &O, int64_t inst, int M, int i, int wl, int n,
                              const int s[4], double z, const FieldRec &r) {
    if (!(A.outs & kOutXC)) return;
    const int64_t at = xc_at(A, inst);
    if (at < 0) return;
    const Dev d = r.dev();
    if (A.outs & kOutX) {
        double *x = O.x + at;
        x[i] = double(wl); x[M + i] = double(n);
        x[2 * M + i] = double(s[0]); x[3 * M + i] = double(s[1]); x[4 * M + i] = double(s[2]);
        x[5 * M + i] = double(s[3]); x[6 * M + i] = z;
    }
    if (A.outs & kOutC) {
        double *c = O.c + at;
        c[i] = d.cw; c[M + i] = d.cn; c[2 * M + i] = d.cs0; c[3 * M + i] = d.cs1; c[4 * M + i] = d.cs2;
        c[5 * M + i] = d.cs3; c[6 * M + i] = 0.0;
    }
}

// The C column of the same solution, x = the largest cycle time and c = k - 1: one lane's pair of stores.
__device__ inline void put_xc_cycle(const SweepArgs &A, const FleetOut &O, int64_t inst, int M, double hmax,
                                    double kc) {
    const int64_t at = xc_at(A, inst);
    if (at >= 0 && (A.outs & kOutX)) O.x[at + 7 * M] = hmax;
    if (at >= 0 && (A.outs & kOutC)) O.c[at + 7 * M] = kc;
}

// x / c of an instance without a solution: its 7 M + 1 entries zeroed by the whole wave.
__device__ inline void zero_xc(const SweepArgs &A, const FleetOut &O, int64_t inst, int M, int lane) {
    const int N = 7 * M + 1;
    const int64_t at = xc_at(A, inst);
    if (at >= 0)
        for (int cc = lane; cc < N; cc += 64) {
            if (A.outs & kOutX) O.x[at + cc] = 0.0;
            if (A.outs & kOutC) O.c[at + cc] = 0.0;
        }
}

#ifndef HALDA_SWEEP_TABLE_K1
#define HALDA_SWEEP_TABLE_K1 1  // table launches also run the k = 1 register greedy (else k = 1 via tables)
#endif

__device__ inline void flag_fleet(const SweepArgs &A, uint8_t *fflag, int f, int lane) {
    // the scratch-free register launch (fflag == nullptr) never flags: sweep_fleets runs it alone only
    // when nothing in the batch can need the table launch (no k > 1 with W >= M, R + 1 <= kDpLanes)
    if (lane == 0 && fflag) {
        fflag[f] = 1;
        __hip_atomic_store(A.hb_flag, A.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ inline void flag_fleet(const SweepArgs &A, int f, int lane) { flag_fleet(A, A.fflag, f, lane); }

// SG = Wave: one fleet per wave; SG = Seg<16>: one fleet (M <= 16, n_k <= 16) per 16-lane segment,
// tables in the segment's LDS slice, k = 1 register greedy and k > 1 incremental threshold scan
// only: what that cannot do (fast-path fallbacks, non-convex / non-monotone leaves) is flagged for
// the one-fleet-per-wave table launch, as the register-only launch does.
// A fleet handed to sweep_fleet with its fields already loaded (the steps kernel, the resident wave): the
// fields of the lane's device, the fleet's first device, and the lane's k_j / W_j.
struct SweepPre {
    DevFields mf;
    int64_t d0;
    int kj, Wj;
};

// F / O: the batch's table and results (the kernel arguments' A.F / A.out, or one batch of a steps
// launch); kPre: the fleet's fields come prefetched in *pre (every fleet has A.uM <= kK1MaxM devices);
// kXC = false: the x / c outputs are compiled out (the caller guarantees outs has none); kLds: A is in
// LDS (the resident wave), its uniform fields arrive in vector registers. Mo: the model the fleet is
// solved for -- the launch's own A.Mo (the overload below), or one variant of a variants launch
// (halda_sweep_variants_kernel), which shares everything else of A.
template <bool kTables, bool kGlobal, class SG = Wave, bool kPre = false, bool kXC = !kPre, bool kLds = false>
__device__ void sweep_fleet(const SweepArgs &A, const halda_fleets &F, const FleetOut &O, int f, const WaveCtx &w,
                            const SG &sg, const SweepPre *pre, const SweepModel &Mo) {
    constexpr int S = SG::S;
    constexpr bool kSeg = S < 64;
    constexpr bool kFirst = !kTables || kSeg;  // a first launch: flags what it leaves to the table launch
    const int lane = sg.sl;  // device index within the fleet
    HALDA_SSTAMP(0, __builtin_amdgcn_s_memtime());
    HALDA_SSTAMP(7, __builtin_amdgcn_s_memrealtime());
    // lane j: k_j and W_j = L / k_j (kernel arguments; their loads are issued with the fields')
    const bool kl = lane < A.n_k;
    const int kj = kPre ? pre->kj : A.ks[kl ? lane : 0];
    const int Wj = kPre ? pre->Wj : kl ? A.Ws[lane] : 0;
    // the fleet's extent: with one fleet size for the batch, from dev_off[0] read through the scalar
    // cache (the table is read-only to the kernel), so that the field loads are the wave's first
    // vector round trip
    // with one fleet size for the batch the first device is dev_off[0] + f uM; dev_off[0] (0 in the
    // usual table) is read beside the field loads below, not in front of them
    int64_t d0 = kPre ? pre->d0 : A.uM > 0 ? int64_t(f) * A.uM : F.dev_off[f];
    const int M = kPre ? A.uM : A.uM > 0 ? A.uM : int(F.dev_off[f + 1] - d0);
    // the outputs this call writes (a steps launch has no x / c: those paths compile out of it)
    const int outs = kXC ? A.outs : A.outs & (kOutObk | kOutSt);
    bool regs = M <= kK1MaxM;  // lane = device: the k = 1 greedy runs in registers
    if constexpr (kSeg || kPre) regs = true;  // the host sends fleets of at most S / kK1MaxM devices
    FieldRec me = {};
    int bad = 0;
    double tsum = 0.0, xsum = 0.0, kappa = 0.0;
    if (regs) {
        // every field of this lane's device in one round trip (lanes past M read device 0). With one
        // fleet size the loads are issued at once from dev_off[0] = 0 (the usual table) while the
        // scalar read of dev_off[0] is in flight, and reissued only where it is not 0: no dependent
        // round trip in front of the field loads.
        DevFields mf = kPre ? pre->mf : load_fields(F, d0 + (lane < M ? lane : 0));
        if (!kPre && A.uM > 0) {
            // a vector read (returns in order behind the field loads: no wait of its own, unlike a
            // scalar read, whose lgkmcnt wait would also hold the kernel-argument reads)
            const int64_t base = __builtin_amdgcn_readfirstlane(int(F.dev_off[0])) |
                                 (int64_t(__builtin_amdgcn_readfirstlane(int(uint64_t(F.dev_off[0]) >> 32))) << 32);
            if (base != 0) {
                d0 += base;
                mf = load_fields(F, d0 + (lane < M ? lane : 0));
            }
        }
        me = field_rec(Mo, mf, bad);
        bad = lane < M ? bad : 0;
        if (M > 0) fleet_offsets_regs<SG, kLds>(Mo, mf, M, sg, tsum, xsum, kappa);
    } else {
        if (A.uM > 0) d0 += sload_i64(F.dev_off);
        for (int i = lane; i < M; i += 64) {
            int b1 = 0;
            field_rec(Mo, load_fields(F, d0 + i), b1);
            bad |= b1;
        }
        fleet_offsets_tree(Mo, F, d0, M, lane, tsum, xsum, kappa);
    }
    bad = sg.any(bad != 0) ? 1 : 0;
    HALDA_SSTAMP(1, __builtin_amdgcn_s_memtime());
#if defined(HALDA_EXIT_AT) && HALDA_EXIT_AT == 1  // diagnostic: VALU of the records phase alone
    if constexpr (!kTables && !kSeg) {
        const double sink = me.alpha + me.b + me.p_bp + me.p_b + me.cst + double(me.Kset + me.Kvram + me.cls + me.gpu) +
                            tsum + xsum + kappa + double(bad);
        if (lane == 0) O.obj_value[f] = sg.sum_f64(sink);
        return;
    }
#endif
    HALDA_SSTAMP(9, __builtin_amdgcn_s_memrealtime());
    double best = kInf;
    int best_k = 0;
    // the k's settled without a solve (the screen's verdicts: W >= 1e6 unsupported, M > W
    // bound-infeasible, rows decode rejects) are written lane-parallel, and the loop below visits only
    // the others, in ascending k
    constexpr int kOpen = 1000;
    int stj = kOpen;
    if (!(Wj < 1000000)) stj = HALDA_STATUS_UNSUPPORTED;
    else if (M > Wj) stj = HALDA_STATUS_INFEASIBLE;  // sum lb(w) = M > W (HiGHS presolve)
    else if (M > 0 && bad) stj = HALDA_STATUS_UNSUPPORTED;
    if (kl && stj != kOpen) {
        const int64_t inst = int64_t(f) * A.n_k + lane;
        if (outs & kOutObk) O.obj_by_k[inst] = kInf;
        if (outs & kOutSt) O.status[inst] = stj;
    }
    if ((outs & kOutXZ) && (outs & kOutXC)) {  // x / c of a settled instance are zero
        uint64_t settled = sg.bits(kl && stj != kOpen);
        const int N = 7 * M + 1;
        while (settled) {
            const int j = __builtin_ctzll(settled);
            settled &= settled - 1;
            const int64_t at = xc_at(A, int64_t(f) * A.n_k + j);
            if (at >= 0)
                for (int cc = lane; cc < N; cc += S) {
                    if (outs & kOutX) O.x[at + cc] = 0.0;
                    if (outs & kOutC) O.c[at + cc] = 0.0;
                }
        }
    }
    uint64_t todo = sg.bits(kl && stj == kOpen);
    const int M_all = M;
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        // the record and M are opaque to the compiler at each k: nothing derived from them is hoisted
        // out of this loop (hoisted per-lane masks and addresses held across the loop spill SGPRs; most
        // fleets open one k)
        opaque_rec(me);
        int M = M_all;
        if constexpr (!kSeg && !kLds) asm volatile("" : "+s"(M));
        const int k = sg.bcast(kj, j);
        const int W = sg.bcast(Wj, j);
        const int64_t inst = int64_t(f) * A.n_k + j;
        const double kc = double(k - 1);
        int st;
        double obj = kInf;
        bool improved = false;
        if (M == 0) st = W > 0 ? HALDA_STATUS_INFEASIBLE : HALDA_STATUS_OPTIMAL;  // x = [C = 0]
        else {
            int rc = K1_FALLBACK, e = 0, rounds = 0, nE = 0;
            double gE = 0.0;
            bool haveE = true;  // gE / nE hold the split at w = 1 + e (k1_alloc), else split here
            me.W = W;
            if (k == 1) HALDA_SSTAMP(2, __builtin_amdgcn_s_memtime());
#if defined(HALDA_EXIT_AT) && HALDA_EXIT_AT == 2  // diagnostic: records + the bookkeeping before the greedy
            if constexpr (!kTables && !kSeg) {
                const double sink = me.alpha + me.b + me.p_bp + me.p_b + me.cst + double(me.Kset + me.Kvram + me.cls +
                                    me.gpu + me.W + k + W) + tsum + xsum + kappa;
                if (lane == 0) O.obj_value[f] = sg.sum_f64(sink);
                return;
            }
#endif
            // k = 1: the register greedy; W = M (R = 0): every w_i = 1 is forced, so the same code gives
            // the solution for any k (the output adds (k - 1) max_i H_i)
            if ((k == 1 || W == M) && regs && (!kTables || HALDA_SWEEP_TABLE_K1 || W == M)) {
                if constexpr (!kTables) {
                    // the register launch solves its greedy fallbacks itself (exact DP, R + 1 <= kDpLanes)
                    if (!A.k1dp) rc = k1_alloc(me, M, W - M, sg, e, rounds, gE, nE);
                    if (rc == K1_FALLBACK && W - M < kDpLanes) {
                        rc = k1_dp(me, M, W - M, sg, e, w.dparg);
                        haveE = false;
                    }
                } else {
                    rc = k1_alloc(me, M, W - M, sg, e, rounds, gE, nE);
                }
            }
            if (k == 1) HALDA_SSTAMP(3, __builtin_amdgcn_s_memtime());
#if defined(HALDA_EXIT_AT) && HALDA_EXIT_AT == 3  // diagnostic: ... + the k = 1 greedy
            if constexpr (!kTables && !kSeg) {
                const double sink = gE + double(e + nE + rounds + rc) + tsum + xsum + kappa;
                if (lane == 0) O.obj_value[f] = sg.sum_f64(sink);
                return;
            }
#endif
            if (rc == K1_INFEASIBLE) {
                st = HALDA_STATUS_INFEASIBLE;
            } else if (rc == K1_OK) {
                double g = 0.0, H = 0.0, z = 0.0;
                int n = 0, sl[4] = {0, 0, 0, 0};
                const int wl = 1 + e;
                // the cycle times only matter through (k - 1) max H and the x output: at k = 1 without x
                // the largest cycle time is not formed (kc * hmax is +0 either way: hmax is finite and
                // >= 0 after a successful split)
                const bool need_h = kc != 0.0 || (outs & kOutX);
                if (lane < M) {
                    if (haveE) {
                        g = gE;
                        n = nE;
                        rec_slacks(me, wl, n, sl);
                    } else {
                        split_full(me, wl, g, n, sl);
                    }
                    if (need_h) {
                        double P, Q;
                        dev_cycle(me, wl, n, sl, P, Q);
                        z = Q > P ? 0.5 * (Q - P) : 0.0;
                        H = Q >= P ? 0.5 * (P + Q) : P;
                    }
                }
                const double hmax = need_h ? fmax(0.0, sg.max_f64(lane < M ? H : 0.0)) : 0.0;
                obj = sg.sum_f64(lane < M ? g : 0.0) + kc * hmax;
                obj = obj + tsum;
                obj = obj + xsum;
                obj = obj + kappa;
                st = HALDA_STATUS_OPTIMAL;
                improved = obj < best;
                if (lane < M) {
                    if (outs & kOutXC) put_xc(A, O, inst, M, lane, wl, n, sl, z, me);
                    if (improved) {
                        O.w[d0 + lane] = wl;
                        O.n[d0 + lane] = n;
                    }
                }
                if (lane == 0 && (outs & kOutXC)) {
                    const int64_t at = xc_at(A, inst);
                    if (at >= 0 && (outs & kOutX)) O.x[at + 7 * M] = hmax;
                    if (at >= 0 && (outs & kOutC)) O.c[at + 7 * M] = kc;
                }
                HALDA_SSTAMP(4, __builtin_amdgcn_s_memtime());
            } else if constexpr (!kTables) {
                // k > 1, a wide fleet or a fast-path fallback: the table launch redoes this fleet
                flag_fleet(A, f, lane);
                return;
            } else {
                if (kSeg && (kc == 0.0 || M < 2)) {  // a k = 1 fast-path fallback / one device: the 64-lane kernel
                    flag_fleet(A, f, lane);
                    return;
                }
                Inst I = {};
                I.inst = int(inst);
                HALDA_TSTAMP(0);
                I.M = M;
                I.W = W;
                I.Wd = double(W);
                I.kc = kc;
                I.iC = 7 * M;
                I.R1 = W - M + 1;
                I.RS = odd_stride(I.R1);
                const FieldSrc src{&Mo, &F, regs ? &me : nullptr, d0, W, sg.base};
                int64_t nodes = 0;
                const bool too_large =
                    M > A.mmax || I.R1 > A.r1max || int64_t(M) * I.RS > (kc > 0.0 ? A.tab_kc : A.tab);
                if (kSeg && too_large) {
                    flag_fleet(A, f, lane);
                    return;
                }
                int feas = 1;
                if (!too_large) {
                    table_pass<S>(src, w, I, lane);
                    wave_sync();
                    HALDA_TSTAMP(6);
                    if constexpr (kSeg) {
                        feas = dp_pass_lanes(w, I, sg, nodes);
                        if (feas < 0) {  // a leaf the incremental scan does not take
                            flag_fleet(A, f, lane);
                            return;
                        }
                    } else {
                        feas = dp_pass(w, I, lane, nodes) ? 1 : 0;
                    }
                }
                if (too_large) {
                    st = HALDA_STATUS_TOO_LARGE;  // beyond the launch's slice (the host sizes it from the fleets)
                } else if (!feas) {
                    st = HALDA_STATUS_INFEASIBLE;
                } else {
                    HALDA_TSTAMP(7);
                    // solution: per device (w, n, least slacks, z), sum of costs, largest cycle time
                    double gs = 0.0, hmax = 0.0;
                    for (int i0 = 0; i0 < M; i0 += S) {
                        const int i = i0 + lane;
                        FieldRec d;
                        src.load(d, w, min(i, M - 1));
                        if (i < M) {
                            const int wl = 1 + w.st0[i];
                            double g = 0.0, P, Q;
                            int n = 0, sl[4] = {0, 0, 0, 0};
                            split_full(d, wl, g, n, sl);
                            dev_cycle(d, wl, n, sl, P, Q);
                            gs += g;
                            hmax = fmax(hmax, Q >= P ? 0.5 * (P + Q) : P);
                            if (outs & kOutXC) put_xc(A, O, inst, M, i, wl, n, sl, Q > P ? 0.5 * (Q - P) : 0.0, d);
                        }
                    }
                    hmax = sg.max_f64(hmax);
                    obj = sg.sum_f64(gs) + kc * hmax;
                    obj = obj + tsum;
                    obj = obj + xsum;
                    obj = obj + kappa;
                    st = HALDA_STATUS_OPTIMAL;
                    improved = obj < best;
                    if (improved)
                        for (int i0 = 0; i0 < M; i0 += S) {
                            const int i = i0 + lane;
                            FieldRec d;
                            src.load(d, w, min(i, M - 1));
                            if (i < M) {
                                const int wl = 1 + w.st0[i];
                                double g;
                                int n = 0, sl[4];
                                split_full(d, wl, g, n, sl);
                                O.w[d0 + i] = wl;
                                O.n[d0 + i] = n;
                            }
                        }
                    if (lane == 0 && (outs & kOutXC)) {
                        const int64_t at = xc_at(A, inst);
                        if (at >= 0 && (outs & kOutX)) O.x[at + 7 * M] = hmax;
                        if (at >= 0 && (outs & kOutC)) O.c[at + 7 * M] = kc;
                    }
                    HALDA_TSTAMP(8);
                }
                wave_sync();  // tables / st0 are rewritten by the next k
            }
        }
        if (st == HALDA_STATUS_OPTIMAL && M == 0) {
            obj = 0.0;  // c.x = 0; no devices: the offsets are empty sums and kappa is undefined
            improved = obj < best;
            if (lane == 0 && (outs & kOutXC)) {
                const int64_t at = xc_at(A, inst);
                if (at >= 0 && (outs & kOutX)) O.x[at] = 0.0;
                if (at >= 0 && (outs & kOutC)) O.c[at] = kc;
            }
        }
        if (improved) {
            best = obj;
            best_k = k;
        }
        if ((outs & kOutXZ) && st != HALDA_STATUS_OPTIMAL) {  // x / c of a non-optimal instance are zero
            const int N = 7 * M + 1;
            const int64_t at = xc_at(A, inst);
            if (at >= 0)
                for (int cc = lane; cc < N; cc += S) {
                    if (outs & kOutX) O.x[at + cc] = 0.0;
                    if (outs & kOutC) O.c[at + cc] = 0.0;
                }
        }
        if (lane == 0) {
            if (outs & kOutObk) O.obj_by_k[inst] = st == HALDA_STATUS_OPTIMAL ? obj : kInf;
            if (outs & kOutSt) O.status[inst] = st;
        }
    }
    HALDA_SSTAMP(5, __builtin_amdgcn_s_memtime());
    if (lane == 0) {
        O.best_k[f] = best_k;
        O.obj_value[f] = best;
        if (kFirst && A.fflag) A.fflag[f] = 0;
    }
    if (best_k == 0)
        for (int i = lane; i < M; i += S) {
            O.w[d0 + i] = 0;
            O.n[d0 + i] = 0;
        }
    HALDA_SSTAMP(6, __builtin_amdgcn_s_memtime());
    HALDA_SSTAMP(8, __builtin_amdgcn_s_memrealtime());
}

template <bool kTables, bool kGlobal, class SG = Wave, bool kPre = false, bool kXC = !kPre, bool kLds = false>
__device__ inline void sweep_fleet(const SweepArgs &A, const halda_fleets &F, const FleetOut &O, int f,
                                   const WaveCtx &w, const SG &sg, const SweepPre *pre = nullptr) {
    sweep_fleet<kTables, kGlobal, SG, kPre, kXC, kLds>(A, F, O, f, w, sg, pre, A.Mo);
}

// Mo: the model of every fleet of the launch (A.Mo, or a variant's); fo: added to the fleet index handed
// to sweep_fleet, the index of the fleet's outputs (0 but for a variants launch, see
// halda_sweep_tables_variants_kernel).
template <bool kTables, bool kGlobal>
__device__ inline void sweep_body(const SweepArgs &A, const SweepBatch &B, unsigned char *slice_base,
                                  const SweepModel &Mo, int fo) {
    const int lane = threadIdx.x;
    if (A.want == 1 && __hip_atomic_load(A.hb_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.launch_id)
        return;
    WaveCtx w = {};
    if constexpr (kTables) w = wave_ctx(slice_base, make_slice(A.mmax, A.r1max, A.tab, A.tab_kc));
    const int S = gridDim.x;
    const int nf = B.F.n_fleets;
    for (int64_t b = blockIdx.x; b < nf; b += int64_t(64) * S) {
        const int64_t mine = b + int64_t(lane) * S;
        uint64_t todo = __ballot(mine < nf && (A.want == 0 || B.fflag[mine] == 1));
        while (todo) {
            const int bit = __builtin_ctzll(todo);
            todo &= todo - 1;
            sweep_fleet<kTables, kGlobal>(A, B.F, B.out, int(b + int64_t(bit) * S) + fo, w, Wave(lane), nullptr, Mo);
        }
    }
}

template <bool kTables, bool kGlobal>
__device__ inline void sweep_body(const SweepArgs &A, const SweepBatch &B, unsigned char *slice_base) {
    sweep_body<kTables, kGlobal>(A, B, slice_base, A.Mo, 0);
}

#ifndef HALDA_SWEEP_WAVES_PER_SIMD
#define HALDA_SWEEP_WAVES_PER_SIMD 4  // occupancy target of the register-only sweep (as the k = 1 kernel)
#endif
#ifndef HALDA_SWEEP_WPB
#define HALDA_SWEEP_WPB 4
#endif
constexpr int kSweepWavesPerBlock = HALDA_SWEEP_WPB;  // fleets per workgroup of the register-only sweep

// The register-only sweep: exactly one fleet per wave, kSweepWavesPerBlock waves per workgroup (a
// quarter of the workgroups to dispatch); no loop, so no kernel argument stays live past its use.
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_kernel(SweepArgs A) {
    // wave-uniform by construction; readfirstlane lets the compiler know (scalar fleet addressing)
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    {
        // the kernel arguments the first branches read, fetched together with one value of every other
        // 64-B line of SweepArgs the wave reads through the scalar cache (the model, the table and
        // result pointers): one round trip instead of one per branch and line (each lgkmcnt wait would
        // otherwise hold the next read back)
        const int nf = A.F.n_fleets, nk = A.n_k, um = A.uM;
        const int64_t *doff = A.F.dev_off;
        const double bp = A.Mo.b_prime;
        const double *tc = A.F.T_cpu;
        const int32_t *ow = A.out.w;
        asm volatile("" ::"s"(nf), "s"(nk), "s"(um), "s"(doff), "s"(bp), "s"(tc), "s"(ow));
    }
    if (f >= A.F.n_fleets) return;
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    sweep_fleet<false, false>(A, A.F, A.out, f, w, Wave(int(threadIdx.x & 63)));
}

// ---------------------------------------------------------------- steps launch
// halda_sweep_steps_kernel: `steps` consecutive batches of register sweeps (halda_fleets_group_launch)
// in ONE launch. Batch t is group entry (first + t) mod n_desc: its own resident table and result
// arrays, so every batch's outputs are those its own halda_sweep_kernel launch writes (the same
// sweep_fleet code on the same fields). The waves stay resident, six per SIMD (78 VGPRs): the items
// (batch t, fleet f) are taken in batch order, wave g takes items g, g + n_waves, ..., so at any time
// the resident waves work on one or two consecutive batches (neighbouring table rows in HBM) and a
// wave waiting for its next fleet's fields leaves the SIMD to the five others. No per-batch fill
// (every wave of a launch loading at once, then every wave computing) and no launch per batch.
// Measured against the alternatives: register prefetch of the next item's fields
// (116 VGPRs, four waves per SIMD), fleet-order items, staggered wave starts -- all slower.
// A (batch, fleet) item that recurs (more batches than group entries) may be solved by two waves at
// once: they compute the same values and every location's last write is the final value, so the
// results are those of consecutive launches. Every batch shares the shape of the first (n_fleets,
// uM <= kK1MaxM devices, the model, the k list, no x / c outputs): the host checks it.
struct StepsDesc {
    halda_fleets F;
    FleetOut out;
    int64_t base;  // dev_off[0] of the batch's table (read once by the host)
};

struct StepsArgs {
    const StepsDesc *desc;
    int n_desc;
    int first;      // (first item's batch) mod n_desc
    int steps;
    uint8_t *fflag;  // k-slot steps: per (group entry, fleet) hand-back flags, n_desc x n_fleets
};

__device__ inline const __attribute__((address_space(4))) StepsDesc &steps_desc(const StepsArgs &G, int b) {
    return reinterpret_cast<const __attribute__((address_space(4))) StepsDesc *>(uintptr_t(G.desc))[b];
}

__device__ inline halda_fleets steps_fleets(const __attribute__((address_space(4))) StepsDesc &d) {
    halda_fleets F;
    F.n_fleets = d.F.n_fleets; F.min_devices = d.F.min_devices; F.max_devices = d.F.max_devices;
    F.dev_off = d.F.dev_off; F.os_class = d.F.os_class; F.flags = d.F.flags;
    F.scpu_b1 = d.F.scpu_b1; F.sgpu_b1 = d.F.sgpu_b1; F.T_cpu = d.F.T_cpu; F.T_gpu = d.F.T_gpu;
    F.t_kvcpy_cpu = d.F.t_kvcpy_cpu; F.t_kvcpy_gpu = d.F.t_kvcpy_gpu; F.t_ram2vram = d.F.t_ram2vram;
    F.t_vram2ram = d.F.t_vram2ram; F.t_comm = d.F.t_comm; F.s_disk = d.F.s_disk;
    F.d_avail_ram = d.F.d_avail_ram; F.c_cpu = d.F.c_cpu; F.c_gpu = d.F.c_gpu; F.d_avail_cuda = d.F.d_avail_cuda;
    F.d_avail_metal = d.F.d_avail_metal; F.swap = d.F.swap;
    return F;
}

__device__ inline FleetOut steps_out(const __attribute__((address_space(4))) StepsDesc &d) {
    FleetOut o;
    o.best_k = d.out.best_k; o.obj_value = d.out.obj_value; o.w = d.out.w; o.n = d.out.n;
    o.obj_by_k = d.out.obj_by_k; o.status = d.out.status; o.x = d.out.x; o.c = d.out.c;
    return o;
}

// halda_sweep_steps_kernel: the group launch's register form -- `steps` batches of register sweeps in ONE
// launch, one wave per (batch, fleet) item (grid = fleet blocks x steps, blockIdx.y the batch). The
// hardware dispatcher starts each next item's wave on whichever SIMD a wave just left, so one batch's
// tail overlaps the next batch's start, and a wave holds no loop state: 67 VGPRs, seven waves per SIMD
// (the resident-wave form with an item loop: 79 VGPRs, six per SIMD, 49 SGPR spills, 12 % slower).
// Every item runs the same sweep_fleet as halda_sweep_kernel on the same fields (kPre: the fields handed
// in; kXC = false: no x / c), so each batch's results are bit-identical to its own launch.
#ifndef HALDA_STEPS_WAVES
#define HALDA_STEPS_WAVES 6  // occupancy floor of the steps kernel (it takes seven at 67 VGPRs)
#endif

__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_STEPS_WAVES) void halda_sweep_steps_kernel(SweepArgs A,
                                                                                                   StepsArgs G) {
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    const int lane = int(threadIdx.x & 63);
    const int nf = A.F.n_fleets, M = A.uM;
    if (f >= nf) return;
    // 32-bit: first < n_desc and blockIdx.y < 65,536 (a 64-bit modulo is ~100 scalar instructions per wave)
    const int b = int((unsigned(G.first) + blockIdx.y) % unsigned(G.n_desc));
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    const Wave wv(lane);
    SweepPre cur;
    const bool kl = lane < A.n_k;
    cur.kj = A.ks[kl ? lane : 0];
    cur.Wj = kl ? A.Ws[lane] : 0;
    cur.d0 = steps_desc(G, b).base + int64_t(f) * M;
    // 32-bit device index: group_check admits tables of at most 2^29 devices here
    cur.mf = load_fields32(steps_fleets(steps_desc(G, b)), uint32_t(cur.d0 + (lane < M ? lane : 0)));
    sweep_fleet<false, false, Wave, true>(A, steps_fleets(steps_desc(G, b)), steps_out(steps_desc(G, b)), f, w, wv,
                                          &cur);
}

// ---------------------------------------------------------------- sub-fleets of a resident table
// An item is (parent fleet of the table, list of local device indices): the fleet of the listed devices in
// list order (halda_solve_subfleets). The item arrays as the kernels see them.
struct SubArgs {
    const int32_t *parent;   // [n_items]
    const int64_t *sub_off;  // [n_items + 1]
    const int32_t *sub_idx;  // [sub_off[n_items]]
};

__device__ inline int sload_i32(const int32_t *p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) int32_t *>(reinterpret_cast<uintptr_t>(p));
}

// halda_sweep_subfleets_kernel: the fused route -- one wave per item, every item of A.uM <= kK1MaxM listed
// devices (A.F is the parent table with n_fleets = the item count; the host sends only shapes whose
// register sweep needs no table launch). The item's parent, list offset and the parent's first device are
// wave-uniform reads through the scalar cache (the item arrays and dev_off are read-only to the kernel);
// lane j's list entry is the wave's first vector round trip, the 18 fields of device dev_off[parent] +
// idx the second (issued together, as load_fields does). From there on the item is a fleet handed to
// sweep_fleet with its fields prefetched (kPre), exactly as the steps kernel and the resident wave hand
// theirs: the same code on the same fields as halda_sweep_kernel runs on the materialised table, so the
// same bits. pre.d0 is the item's offset in the w / n outputs (sub_off lays them out).
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_subfleets_kernel(
    SweepArgs A, SubArgs S) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    if (i >= A.F.n_fleets) return;
    const int lane = int(threadIdx.x & 63);
    const int M = A.uM;
    const int64_t so = sload_i64(S.sub_off + i);
    const int64_t base = sload_i64(A.F.dev_off + sload_i32(S.parent + i));
    const int idx = S.sub_idx[so + (lane < M ? lane : 0)];
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    SweepPre pre;
    const bool kl = lane < A.n_k;
    pre.kj = A.ks[kl ? lane : 0];
    pre.Wj = kl ? A.Ws[lane] : 0;
    pre.d0 = so;
    pre.mf = load_fields(A.F, base + idx);
    sweep_fleet<false, false, Wave, true, true>(A, A.F, A.out, i, w, Wave(lane), &pre);
}

// halda_expand_subfleets_kernel: the expansion route -- one wave per item copies the 18 fields of its
// listed devices into a compact fleet table E whose dev_off is sub_off itself (item i owns entries
// sub_off[i] .. sub_off[i + 1] - 1); lists longer than a wave take several passes. The ordinary sweep
// then runs on E.
struct ExpandOut {
    uint8_t *os_class, *flags;
    double *f[16];  // the table's double fields in halda_fleets order (scpu_b1 .. swap)
};

__global__ __launch_bounds__(256) void halda_expand_subfleets_kernel(halda_fleets T, SubArgs S, int n_items,
                                                                       ExpandOut E) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    if (i >= n_items) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t so = sload_i64(S.sub_off + i);
    const int len = int(sload_i64(S.sub_off + i + 1) - so);
    const int64_t base = sload_i64(T.dev_off + sload_i32(S.parent + i));
    for (int j = lane; j < len; j += 64) {
        const int64_t g = base + S.sub_idx[so + j], o = so + j;
        const DevFields d = load_fields(T, g);
        E.os_class[o] = uint8_t(d.cls);
        E.flags[o] = uint8_t(d.flags);
        E.f[0][o] = d.scpu; E.f[1][o] = d.sgpu; E.f[2][o] = d.Tc; E.f[3][o] = d.Tg; E.f[4][o] = d.tkc;
        E.f[5][o] = d.tkg; E.f[6][o] = d.r2v; E.f[7][o] = d.v2r; E.f[8][o] = d.tcomm; E.f[9][o] = d.sdisk;
        E.f[10][o] = d.ram; E.f[11][o] = d.ccpu; E.f[12][o] = d.cgpu; E.f[13][o] = d.cuda; E.f[14][o] = d.metal;
        E.f[15][o] = d.swap;
    }
}

// ---------------------------------------------------------------- exact device selection: all subsets
// halda_solve_subsets: the candidates of a fleet are the fleet without d of its droppable devices, kept
// devices in their order; a candidate is a 64-bit combo over droppable SLOTS (bit r: drop the r-th
// droppable device). The host lays out, per d, one SubsetFleet per fleet and one combo list per (q, d) in
// enumeration order (ascending index lists, lexicographic); every launch below works on one d and on the
// items [i0, i0 + n) of that d's item numbering.
struct SubsetFleet {
    int64_t item_off;    // the fleet's first item of this d (fused: f * cmax, expansion: compact prefix)
    int64_t combo_off;   // its (q, d) combo list in SubsetArgs::combos
    int64_t list_off;    // expansion: listed devices of every item in front of the fleet's first
    uint64_t drop_mask;  // its droppable devices
    int32_t cnt;         // its candidates of this d (0: d is beyond what the fleet may drop)
    int32_t M;           // its devices
};

struct SubsetArgs {
    const SubsetFleet *fl;   // [n_fleets] of this d
    const uint64_t *combos;  // every (q, d) list of the call
    int64_t i0;              // the launch's first item
    int64_t l0;              // expansion: listed devices in front of item i0
    int32_t n;               // its items
    int32_t cmax;            // fused: item slots per fleet (slots past cnt run nothing)
    int32_t n_fleets, d;
};

__device__ inline uint64_t sload_u64(const uint64_t *p) {
    return uint64_t(sload_i64(reinterpret_cast<const int64_t *>(p)));
}

__device__ inline SubsetFleet subset_fleet(const SubsetArgs &U, int f) {
    const int64_t *p = reinterpret_cast<const int64_t *>(U.fl + f);
    SubsetFleet s;
    s.item_off = sload_i64(p);
    s.combo_off = sload_i64(p + 1);
    s.list_off = sload_i64(p + 2);
    s.drop_mask = uint64_t(sload_i64(p + 3));
    const int64_t cm = sload_i64(p + 4);
    s.cnt = int32_t(uint32_t(uint64_t(cm)));
    s.M = int32_t(uint64_t(cm) >> 32);
    return s;
}

// Lane j < M - d: the parent index of the j-th kept device of the candidate (lanes past it: that of lane
// 0). Lane = parent device; its slot is the number of droppable devices below it; it is kept unless it is
// droppable and its combo bit is set. Kept lanes push their index forward to their rank among the kept,
// the others (dropped, or past M) to the lanes behind the kept ones: a permutation, every lane active.
__device__ inline int subset_kept_index(uint64_t drop_mask, uint64_t combo, int M, int lane, int *n_kept) {
    const uint64_t below = (uint64_t(1) << lane) - 1;
    const int slot = __popcll(drop_mask & below);
    const bool kept = lane < M && !(((drop_mask >> lane) & 1) && ((combo >> slot) & 1));
    const uint64_t km = __ballot(kept);
    const int nk = __popcll(km);
    const int dest = kept ? __popcll(km & below) : nk + __popcll(~km & below);
    const int got = __builtin_amdgcn_ds_permute(dest << 2, lane);
    *n_kept = nk;
    return lane < nk ? got : __builtin_amdgcn_readfirstlane(got);
}

// halda_sweep_subsets_kernel: the fused route -- one wave per (fleet, candidate) of one d, every fleet of
// M = A.uM + d devices (A.uM = M - d is the candidates' length; the host sends only shapes whose register
// sweep needs no table launch, the sub-fleet kernel's gate). Item g = i0 + wave is (fleet g / cmax,
// candidate g % cmax); the fleet's record and the combo are wave-uniform reads through the scalar cache.
// The kept devices' fields are loaded by the compacted lanes and handed to sweep_fleet (kPre) as
// halda_sweep_subfleets_kernel hands its gathered fields: the same code on the same fields, so the same
// bits as halda_solve_subfleets of the candidate's list. Only best_k / obj_value per item are kept
// (A.out over the launch's items); w / n go to a ring of 64-entry strips nobody reads (ring_mask).
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_subsets_kernel(
    SweepArgs A, SubsetArgs U, int ring_mask) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    if (i >= U.n) return;
    const int lane = int(threadIdx.x & 63);
    const uint32_t g = uint32_t(U.i0) + uint32_t(i);  // the host sends n_fleets * cmax < 2^31 (a 32-bit division)
    const int f = int(g / uint32_t(U.cmax));
    const int cand = int(g - uint32_t(f) * uint32_t(U.cmax));
    const SubsetFleet sf = subset_fleet(U, f);
    if (cand >= sf.cnt) return;
    const uint64_t combo = sload_u64(U.combos + sf.combo_off + cand);
    const int64_t base = sload_i64(A.F.dev_off + f);
    int nk;
    const int idx = subset_kept_index(sf.drop_mask, combo, sf.M, lane, &nk);
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    SweepPre pre;
    const bool kl = lane < A.n_k;
    pre.kj = A.ks[kl ? lane : 0];
    pre.Wj = kl ? A.Ws[lane] : 0;
    pre.d0 = int64_t(i & ring_mask) * 64;
    pre.mf = load_fields(A.F, base + idx);
    sweep_fleet<false, false, Wave, true, false>(A, A.F, A.out, i, w, Wave(lane), &pre);
}

// halda_subsets_index_kernel: the expansion route -- one wave per item writes the candidate as an item of
// halda_solve_subfleets (parent, sub_off, the kept devices' indices) over the launch's items; the fleet of
// item g is the last one whose item_off is <= g (a binary search over uniform reads).
__global__ __launch_bounds__(256) void halda_subsets_index_kernel(SubsetArgs U, int32_t *parent, int64_t *sub_off,
                                                                  int32_t *sub_idx) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    if (i >= U.n) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t g = U.i0 + i;
    int lo = 0, hi = U.n_fleets - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sload_i64(&U.fl[mid].item_off) <= g) lo = mid;
        else hi = mid - 1;
    }
    const SubsetFleet sf = subset_fleet(U, lo);
    const int64_t cand = g - sf.item_off;
    const uint64_t combo = sload_u64(U.combos + sf.combo_off + cand);
    int nk;
    const int idx = subset_kept_index(sf.drop_mask, combo, sf.M, lane, &nk);
    const int64_t so = sf.list_off + cand * int64_t(sf.M - U.d) - U.l0;
    if (lane < nk) sub_idx[so + lane] = idx;
    if (lane == 0) {
        parent[i] = lo;
        sub_off[i] = so;
        if (i == U.n - 1) sub_off[i + 1] = so + nk;
    }
}

// halda_subsets_pick_kernel: one workgroup per fleet -- the arg-min of the launch's items of the fleet's
// group (this d) on (obj_value, candidate index), lexicographic with strict <, so the earliest candidate
// among equal objectives: per thread over its candidates in ascending order, a wave reduction, then one
// over the workgroup's waves through LDS. Folded into the frontier entry where the group began in an
// earlier launch (strict <: the earlier launch's candidates come first). A group without candidates, or
// whose candidates are all infeasible, gets INFEASIBLE, +inf and mask 0.
struct SubsetFrontier {
    int32_t *status;
    double *obj;
    uint64_t *dropped_mask;
    int32_t *best_k;
};

__device__ inline void subset_min(double &o, int64_t &c, double o2, int64_t c2) {
    if (c2 >= 0 && (c < 0 || o2 < o || (o2 == o && c2 < c))) {
        o = o2;
        c = c2;
    }
}

__global__ __launch_bounds__(256) void halda_subsets_pick_kernel(SubsetArgs U, const double *obj, const int32_t *best_k,
                                                                 SubsetFrontier R, int stride) {
    const int f = int(blockIdx.x);
    const SubsetFleet sf = subset_fleet(U, f);
    const int64_t a = sf.item_off > U.i0 ? sf.item_off : U.i0;
    const int64_t e = sf.item_off + sf.cnt, lim = U.i0 + U.n;
    const int64_t b = e < lim ? e : lim;
    const int64_t at = int64_t(f) * stride + U.d;
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
    for (int64_t g = a + threadIdx.x; g < b; g += 256) subset_min(o, c, obj[g - U.i0], g - sf.item_off);
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
    if (a > sf.item_off && !(o < R.obj[at])) return;  // the group began earlier: only a strictly lower value moves it
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
    R.best_k[at] = best_k[sf.item_off + c - U.i0];
}

// ---------------------------------------------------------------- model variants of one table
// halda_solve_variants: one fleet table solved for n_var models in one launch, blockIdx.y the variant.
// The variants share the table, the k list, L (so every W = L / k and the plan's shapes) and has_f_q /
// has_f_out; everything else of the model is per variant: the call's SweepModel array (bvo formed on the
// host per variant, as A.Mo.bvo is) in context scratch, read-only to the kernel, so a wave reads its
// variant's model through the scalar cache, as the steps kernels read their batch's descriptor.
// The outputs are variant-major, which is the layout of a batch of n_var * n_fleets fleets: variant v's
// fleet f is output fleet v * n_fleets + f for best_k / obj_value / obj_by_k / status / x / c / x_off
// (sweep_fleet's fleet index), and its devices' w / n lie at v * dev_off[n_fleets] + their table index.
struct VarArgs {
    const SweepModel *models;  // [n_var]
};

__device__ inline SweepModel var_model(const VarArgs &V, int v) {
    const __attribute__((address_space(4))) SweepModel &m =
        reinterpret_cast<const __attribute__((address_space(4))) SweepModel *>(uintptr_t(V.models))[v];
    SweepModel o;
    o.f_q_b1 = m.f_q_b1; o.f_out_b1 = m.f_out_b1; o.has_f_q = m.has_f_q; o.has_f_out = m.has_f_out;
    o.b_prime = m.b_prime; o.b_layer = m.b_layer; o.b_in = m.b_in; o.b_out = m.b_out; o.V = m.V; o.L = m.L;
    o.bvo = m.bvo;
    return o;
}

// halda_sweep_variants_kernel: the register form -- one wave per (variant, fleet), every fleet of
// A.uM <= kK1MaxM devices and a plan that needs no table launch (the host checks both). The fleet's fields
// are loaded as halda_sweep_kernel loads them and handed to the same sweep_fleet (kPre, as the sub-fleet
// kernel hands its gathered fields), with the variant's model: the same code on the same fields and
// model as that variant's own halda_sweep_kernel launch, so the same bits. pre.d0 is where the fleet's
// w / n go.
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_variants_kernel(
    SweepArgs A, VarArgs V) {
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    const int nf = A.F.n_fleets;
    if (f >= nf) return;
    const int v = int(blockIdx.y);
    const int lane = int(threadIdx.x & 63);
    const int M = A.uM;
    const int64_t base = sload_i64(A.F.dev_off), nd = sload_i64(A.F.dev_off + nf);
    const SweepModel Mo = var_model(V, v);
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    SweepPre pre;
    const bool kl = lane < A.n_k;
    pre.kj = A.ks[kl ? lane : 0];
    pre.Wj = kl ? A.Ws[lane] : 0;
    const int64_t d0 = base + int64_t(f) * M;
    pre.d0 = int64_t(v) * nd + d0;
    pre.mf = load_fields(A.F, d0 + (lane < M ? lane : 0));
    sweep_fleet<false, false, Wave, true, true>(A, A.F, A.out, v * nf + f, w, Wave(lane), &pre, Mo);
}

// ---------------------------------------------------------------- a caller's plan priced on the table
// halda_eval_plans: fleet f's plan (k, w[M], n[M]) evaluated on the fleet's records at W = L / k -- the
// least slacks (rec_slacks), the device cost (rec_try's expression), the cycle time (dev_cycle) and the
// objective sweep_fleet forms, on the caller's (w, n) instead of on the minimiser.
// reason bits of an infeasible plan:
constexpr int kPlanSumW = 1;     // sum w != W
constexpr int kPlanRangeW = 2;   // some w_i outside [1, W]
constexpr int kPlanRangeN = 4;   // some n_i outside its interval (rec_interval at w_i)
constexpr int kPlanSlack = 8;    // a slack over its bound: setok false, or the VRAM slack over nhi
constexpr int kPlanRecord = 16;  // record rejected (bad / rec_nanx), or W >= 1e6: HALDA_STATUS_UNSUPPORTED
constexpr int kPlanNone = 32;    // k <= 0: no plan
// PlanArgs.outs: the optional outputs wanted (kOutX / kOutC and these)
constexpr int kPlanOutCycle = 32, kPlanOutBott = 64, kPlanOutReason = 128;

struct PlanArgs {
    const int32_t *k, *w, *n;  // halda_plans
    int32_t *status;           // halda_plan_result
    double *obj_value, *cycle;
    int32_t *bottleneck, *reason;
    double *x, *c;
    const int64_t *x_off;
    int64_t xstride;  // dense x / c: 7 max_devices + 1 per fleet
    int outs;
};

// One device of a plan: its reason bits, and where it has none its cost g (rec_try's term order), least
// slacks s, least cycle time H and z as sweep_fleet forms them for a solved k. W is 0 for a plan without
// a usable k (every w is then out of range); the n checks are made only where w_i is in [1, W] < 1e6, so
// no sum below can leave the int range whatever the caller's w / n hold.
struct PlanDev {
    double g, H, z;
    int s[4];
    int reason;
};

__device__ inline PlanDev plan_dev(FieldRec &r, int bad, int W, int wl, int n) {
    PlanDev d;
    d.g = 0.0; d.H = 0.0; d.z = 0.0;
    d.s[0] = d.s[1] = d.s[2] = d.s[3] = 0;
    r.W = W;
    int reason = (bad || rec_nanx(r)) ? kPlanRecord : 0;
    const bool wok = wl >= 1 && wl <= W;
    if (!wok) reason |= kPlanRangeW;
    if (wok) {
        int nL, nU;
        rec_interval(r, wl, nL, nU);
        const bool hs = r.Kset != kNoRow;
        const bool setok = !(hs && (r.cls == 1 || r.cls == 2)) || max(0, wl + r.Kset) <= W;
        const int nhi = r.gpu ? W : 0;
        if (!(n >= nL && n <= nU)) reason |= kPlanRangeN;
        if (!setok || (r.Kvram != kNoRow && n > nhi - r.Kvram)) reason |= kPlanSlack;
    }
    d.reason = reason;
    if (reason == 0) {
        rec_slacks(r, wl, n, d.s);
        const double pv = rec_pv(r), pvo = rec_own(r) ? pv : 0.0;
        const int sc = max(0, wl - (r.cls == 3 ? n : 0) + r.Kset);
        double g = r.alpha * double(wl);
        g = g + r.b * double(n);
        g = g + pvo * double(sc);
        g = g + pv * double(d.s[3]);
        d.g = g;
        double P, Q;
        dev_cycle(r, wl, n, d.s, P, Q);
        d.z = Q > P ? 0.5 * (Q - P) : 0.0;
        d.H = Q >= P ? 0.5 * (P + Q) : P;
    }
    return d;
}

// Column i of the plan's x / c (put_xc's layout [w|n|s1|s2|s3|t|z|C]); zeros for a plan that is not feasible.
__device__ inline void plan_put_xc(const PlanArgs &E, int64_t at, int M, int i, bool feas, int wl, int n,
                                   const PlanDev &d, const FieldRec &r) {
    if (E.outs & kOutX) {
        double *x = E.x + at;
        x[i] = feas ? double(wl) : 0.0; x[M + i] = feas ? double(n) : 0.0;
        x[2 * M + i] = double(feas ? d.s[0] : 0); x[3 * M + i] = double(feas ? d.s[1] : 0);
        x[4 * M + i] = double(feas ? d.s[2] : 0); x[5 * M + i] = double(feas ? d.s[3] : 0);
        x[6 * M + i] = feas ? d.z : 0.0;
    }
    if (E.outs & kOutC) {
        double *c = E.c + at;
        c[i] = feas ? r.alpha : 0.0; c[M + i] = feas ? r.b : 0.0; c[2 * M + i] = feas ? r.p_bp : 0.0;
        c[3 * M + i] = feas ? r.p_b : 0.0; c[4 * M + i] = feas ? r.p_bp : 0.0;
        c[5 * M + i] = feas ? rec_pv(r) : 0.0; c[6 * M + i] = 0.0;
    }
}

// The fleet's verdict from the OR of its devices' reason bits, sum w (a double: exact for any int32 w) and k.
__device__ inline int plan_reason(int dev_bits, double wsum, int k, int W) {
    if (k <= 0) return kPlanNone;
    int reason = dev_bits;
    if (!(W < 1000000)) reason |= kPlanRecord;
    if (wsum != double(W)) reason |= kPlanSumW;
    return reason;
}

__device__ inline void plan_store(const PlanArgs &E, int f, int64_t at, int M, int lane, int reason, double obj,
                                  double C, double hraw, int bott, int k) {
    const bool feas = reason == 0;
    if (lane == 0) {
        E.status[f] = feas ? HALDA_STATUS_OPTIMAL
                           : (reason & kPlanRecord) ? HALDA_STATUS_UNSUPPORTED : HALDA_STATUS_INFEASIBLE;
        E.obj_value[f] = feas ? obj : kInf;
        if (E.outs & kPlanOutCycle) E.cycle[f] = feas ? C : kInf;
        if (E.outs & kPlanOutBott) E.bottleneck[f] = feas && hraw > 0.0 ? bott : -1;
        if (E.outs & kPlanOutReason) E.reason[f] = reason;
        if (at >= 0 && (E.outs & kOutX)) E.x[at + 7 * M] = feas ? C : 0.0;
        if (at >= 0 && (E.outs & kOutC)) E.c[at + 7 * M] = feas ? double(k - 1) : 0.0;
    }
}

__device__ inline int64_t plan_xc_at(const PlanArgs &E, int f) {
    if (!(E.outs & kOutXC)) return -1;
    return E.x_off ? E.x_off[f] : int64_t(f) * E.xstride;
}

// A fleet of M <= 64 devices, lane = device, its fields (mf), plan entries (pw, pn) and k already loaded.
// The objective is added in sweep_fleet<.., Wave>'s order: sum_f64(g) + kc hmax, + tsum, + xsum, + kappa
// (fleet_offsets_regs's constants), so a plan that is a sweep's own (k, w, n) gets the sweep's bits.
__device__ inline void eval_plan_regs(const SweepModel &Mo, const PlanArgs &E, int f, int M, const Wave &sg,
                                      const DevFields &mf, int k, int pw, int pn) {
    const int lane = sg.sl;
    const bool act = lane < M;
    int bad = 0;
    FieldRec r = field_rec(Mo, mf, bad);
    const int Wk = k > 0 ? Mo.L / k : 0;
    const int W = Wk < 1000000 ? Wk : 0;
    const PlanDev d = plan_dev(r, bad, W, pw, pn);
    const int reason = plan_reason(sg.or_i(act ? d.reason : 0), sg.sum_f64(act ? double(pw) : 0.0), k, Wk);
    const bool feas = reason == 0;
    double tsum, xsum, kappa;
    fleet_offsets_regs<Wave, false>(Mo, mf, M, sg, tsum, xsum, kappa);
    const double hraw = sg.max_f64(act && feas ? d.H : -kInf);
    const double C = fmax(0.0, hraw);
    const int bott = sg.lowest(act && d.H == hraw);
    double obj = sg.sum_f64(act ? d.g : 0.0) + double(k - 1) * C;
    obj = obj + tsum;
    obj = obj + xsum;
    obj = obj + kappa;
    const int64_t at = plan_xc_at(E, f);
    if (at >= 0 && act) plan_put_xc(E, at, M, lane, feas, pw, pn, d, r);
    plan_store(E, f, at, M, lane, reason, obj, C, hraw, bott, k);
}

// A fleet wider than a wave: 64-device chunks, the partial sums, max and its lowest device carried in
// registers (a lane's devices come in ascending order, so a strict ">" keeps the lowest), the constants
// from fleet_offsets_tree -- the table path's order in sweep_fleet. x / c need the fleet's verdict first:
// a second pass over the chunks rebuilds each device's values (no per-device state is kept).
__device__ inline void eval_plan_wide(const SweepModel &Mo, const halda_fleets &F, const PlanArgs &E, int f,
                                      int64_t d0, int M, const Wave &sg, int k) {
    const int lane = sg.sl;
    const int Wk = k > 0 ? Mo.L / k : 0;
    const int W = Wk < 1000000 ? Wk : 0;
    double gs = 0.0, ws = 0.0, hm = -kInf;
    int bits = 0, bi = 0x7fffffff;
    for (int i = lane; i < M; i += 64) {
        int bad = 0;
        const DevFields mf = load_fields(F, d0 + i);
        const int pw = E.w[d0 + i], pn = E.n[d0 + i];
        FieldRec r = field_rec(Mo, mf, bad);
        const PlanDev d = plan_dev(r, bad, W, pw, pn);
        bits |= d.reason;
        ws += double(pw);
        gs += d.g;
        if (d.reason == 0 && d.H > hm) {
            hm = d.H;
            bi = i;
        }
    }
    const int reason = plan_reason(sg.or_i(bits), sg.sum_f64(ws), k, Wk);
    const bool feas = reason == 0;
    double tsum, xsum, kappa;
    fleet_offsets_tree(Mo, F, d0, M, lane, tsum, xsum, kappa);
    const double hraw = sg.max_f64(hm);
    const double C = fmax(0.0, hraw);
    const int bott = sg.imin(hm == hraw ? bi : 0x7fffffff);
    double obj = sg.sum_f64(gs) + double(k - 1) * C;
    obj = obj + tsum;
    obj = obj + xsum;
    obj = obj + kappa;
    const int64_t at = plan_xc_at(E, f);
    if (at >= 0)
        for (int i = lane; i < M; i += 64) {
            int bad = 0;
            const int pw = E.w[d0 + i], pn = E.n[d0 + i];
            FieldRec r = field_rec(Mo, load_fields(F, d0 + i), bad);
            const PlanDev d = plan_dev(r, bad, W, pw, pn);
            plan_put_xc(E, at, M, i, feas, pw, pn, d, r);
        }
    plan_store(E, f, at, M, lane, reason, obj, C, hraw, bott, k);
}

struct EvalArgs {
    SweepModel Mo;
    halda_fleets F;
    PlanArgs E;
};

// halda_eval_plans_kernel: the general route -- one wave per fleet, four per workgroup, any fleet size.
// The fleet's extent and the plan's k are wave-uniform reads through the scalar cache (read-only to the
// kernel); the plan's w / n are two 4-byte loads issued with the 18 field loads. No LDS.
__global__ __launch_bounds__(256) void halda_eval_plans_kernel(EvalArgs A) {
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    if (f >= A.F.n_fleets) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t d0 = sload_i64(A.F.dev_off + f);
    const int M = int(sload_i64(A.F.dev_off + f + 1) - d0);
    const int k = sload_i32(A.E.k + f);
    const Wave sg(lane);
    if (M <= 0) {  // no devices: nothing to read
        plan_store(A.E, f, -1, 0, lane, k <= 0 ? kPlanNone : kPlanSumW, kInf, kInf, 0.0, -1, k);
        return;
    }
    if (M <= kK1MaxM) {
        const int64_t g = d0 + (lane < M ? lane : 0);
        const DevFields mf = load_fields(A.F, g);
        const int pw = A.E.w[g], pn = A.E.n[g];
        eval_plan_regs(A.Mo, A.E, f, M, sg, mf, k, pw, pn);
    } else {
        eval_plan_wide(A.Mo, A.F, A.E, f, d0, M, sg, k);
    }
}

// halda_sweep_plans_kernel: the fused route -- the register sweep of a batch of fleets of one size
// A.uM <= kK1MaxM that needs no table launch (the host checks both), with the incumbent plan priced on the
// sweep's own field loads: the wave loads its fleet's fields once (the plan's w / n with them), evaluates
// the plan and stores its outputs, and only then hands the same fields to the unedited sweep_fleet (kPre,
// as the sub-fleet and variants kernels hand theirs) -- nothing of the evaluation is live across the sweep.
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_plans_kernel(
    SweepArgs A, PlanArgs E) {
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    if (f >= A.F.n_fleets) return;
    const int lane = int(threadIdx.x & 63);
    const int M = A.uM;
    const int64_t base = sload_i64(A.F.dev_off);
    const int k = sload_i32(E.k + f);
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    SweepPre pre;
    const bool kl = lane < A.n_k;
    pre.kj = A.ks[kl ? lane : 0];
    pre.Wj = kl ? A.Ws[lane] : 0;
    pre.d0 = base + int64_t(f) * M;
    const int64_t g = pre.d0 + (lane < M ? lane : 0);
    pre.mf = load_fields(A.F, g);
    const int pw = E.w[g], pn = E.n[g];
    const Wave sg(lane);
    eval_plan_regs(A.Mo, E, f, M, sg, pre.mf, k, pw, pn);
    sweep_fleet<false, false, Wave, true, true>(A, A.F, A.out, f, w, sg, &pre);
}

// ---------------------------------------------------------------- per-device layer bounds
// halda_solve_fleets_bounded: the k-sweep with the w columns' bounds narrowed from [1, W] to
// [lo_i, hi_i] = [max(1, w_min_i), min(W, w_max_i)]; n, the slacks, z, C and every row
// stay as they are. Either array may be absent (nullptr: no bound on that side).
struct BoundArgs {
    const int32_t *w_min, *w_max;  // halda_bounds: [dev_off[n_fleets]] device layout
};
struct BoxArgs {
    const int32_t *w_min, *w_max, *n_min, *n_max;  // halda_box: the same layout
};

// Capped bound sums: every open W is < 1e6 < kBoundCap, so sum min(b_i, kBoundCap) compares with W as the
// uncapped sum does, and 4096 capped terms of a lane's share / 64 lane sums stay inside an int.
constexpr int kBoundCap = 1 << 24;

// The general route's patch of a lowered batch (halda_lower_kernel's layout: instance (f, j) has its
// columns at (f n_k + j) cols, the w columns first): one wave per instance, lane = column, col_lb / col_ub
// of the M w columns overwritten with lo / hi. lo is capped at W + 1 (any lo > W is infeasible by itself,
// the screen's rule), so the screen's integer sum of the lower bounds stays small.
// Args = BoxArgs (halda_solve_fleets_boxed with n bounds; halda_box_cols_kernel is launched INSTEAD of
// halda_bound_cols_kernel): the w columns get the folded lo = max(1, w_min, nlo) (an implied bound through
// the link row n <= w, so the screen's sum of lower bounds is the fused routes' sum lo), the n columns
// nlo = max(0, n_min) and min(the lowering's own upper bound, n_max). A crossing n pair is written as it
// is: n_interval then finds no n at any w, every table entry of the device is +inf, the leaf is empty and
// the instance INFEASIBLE.
template <class Args>
__device__ inline void bound_cols(const halda_fleets &F, const Args &Bd, const int32_t *ks, int n_k, int L,
                                  int64_t cols, double *col_lb, double *col_ub) {
    constexpr bool kBox = std::is_same<Args, BoxArgs>::value;
    const int64_t inst = int64_t(blockIdx.x) * 4 + int(threadIdx.x >> 6);
    if (inst >= int64_t(F.n_fleets) * n_k) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t f = inst / n_k;
    const int j = int(inst - f * n_k);
    const int64_t d0 = F.dev_off[f];
    const int M = int(F.dev_off[f + 1] - d0);
    const int W = L / ks[j];
    const int64_t co = inst * cols;
    for (int i = lane; i < M; i += 64) {
        int nlo = 0, nmx = 0x7fffffff;
        if constexpr (kBox) {
            nlo = max(0, Bd.n_min ? Bd.n_min[d0 + i] : 0);
            nmx = Bd.n_max ? Bd.n_max[d0 + i] : 0x7fffffff;
        }
        const int lo = max(max(1, Bd.w_min ? Bd.w_min[d0 + i] : 0), nlo);
        const int hi = Bd.w_max ? Bd.w_max[d0 + i] : 0x7fffffff;
        col_lb[co + i] = lo > W ? double(W) + 1.0 : double(lo);
        col_ub[co + i] = double(min(W, hi));
        if constexpr (kBox) {
            col_lb[co + M + i] = double(nlo);
            col_ub[co + M + i] = fmin(col_ub[co + M + i], double(nmx));
        }
    }
}

__global__ __launch_bounds__(256) void halda_bound_cols_kernel(halda_fleets F, BoundArgs Bd, const int32_t *ks, int n_k,
                                                               int L, int64_t cols, double *col_lb, double *col_ub) {
    bound_cols(F, Bd, ks, n_k, L, cols, col_lb, col_ub);
}

__global__ __launch_bounds__(256) void halda_box_cols_kernel(halda_fleets F, BoxArgs Bx, const int32_t *ks, int n_k, int L,
                                                             int64_t cols, double *col_lb, double *col_ub) {
    bound_cols(F, Bx, ks, n_k, L, cols, col_lb, col_ub);
}

// The compact record with its w bounds: k1_alloc, k1_dp and the splits read a record's bounds through
// rec_wlo / rec_whi and its broadcast form through bcast() / core(), so the register greedy and its exact
// DP fallback run on [wlo, whi] unedited (split_first / split_second fall back to split_full where the
// lower bound is not 1). With wlo = 1, whi = W every value equals the FieldRec's.
struct UBoundRec : UFieldRec {
    int wlo, whi;
    __device__ inline const UBoundRec &core() const { return *this; }
};

struct BoundRec : FieldRec {
    int wlo, whi;
    template <class SG>
    __device__ inline UBoundRec bcast(const SG &sg, int src) const {
        UBoundRec o;
        static_cast<UFieldRec &>(o) = FieldRec::bcast(sg, src);
        o.wlo = sg.bcast(wlo, src);
        o.whi = sg.bcast(whi, src);
        return o;
    }
    __device__ inline const BoundRec &core() const { return *this; }
};

__device__ inline int rec_wlo(const BoundRec &r) { return r.wlo; }
__device__ inline int rec_whi(const BoundRec &r) { return r.whi; }
__device__ inline int rec_wlo(const UBoundRec &r) { return r.wlo; }
__device__ inline int rec_whi(const UBoundRec &r) { return r.whi; }

// halda_solve_fleets_boxed: the bounded record with a box on n beside [wlo, whi] -- n in [nlo, nhi],
// nlo = max(0, n_min_i), nhi = n_max_i as given (rec_interval's own nU is already <= the reference's
// nhi_i, so the minimum with it is taken there). The upper bound of the VRAM slack t stays the reference's
// nhi_i = (gpu ? W : 0): the box narrows n, not t, so rec_interval's nhi_i - Kvram term is the FieldRec's.
// A box record is a BoundRec, so rec_wlo / rec_whi, rec_try, rec_slacks and dev_cycle are the bounded
// record's; only the n-interval, and with it the four splits, are its own.
struct UBoxRec : UBoundRec {
    int nlo, nhi;
    __device__ inline const UBoxRec &core() const { return *this; }
};

struct BoxRec : BoundRec {
    int nlo, nhi;
    template <class SG>
    __device__ inline UBoxRec bcast(const SG &sg, int src) const {
        UBoxRec o;
        static_cast<UBoundRec &>(o) = BoundRec::bcast(sg, src);
        o.nlo = sg.bcast(nlo, src);
        o.nhi = sg.bcast(nhi, src);
        return o;
    }
    __device__ inline const BoxRec &core() const { return *this; }
};

// The FieldRec's interval clamped into [nlo, nhi] after everything it does: the intersection of two
// intervals, empty (false) when either is or when they do not meet.
template <class R>
__device__ inline bool box_interval(const R &r, int w, int &nL, int &nU) {
    const bool ok = rec_interval(static_cast<const FieldRec &>(r), w, nL, nU);
    nL = max(nL, r.nlo);
    nU = min(nU, r.nhi);
    return ok & (nL <= nU);
}
__device__ inline bool rec_interval(const BoxRec &r, int w, int &nL, int &nU) { return box_interval(r, w, nL, nU); }
__device__ inline bool rec_interval(const UBoxRec &r, int w, int &nL, int &nU) { return box_interval(r, w, nL, nU); }

// The splits on a box record: the FieldRec's bodies (the same candidates, tie rule and term order) on the
// clamped interval. The cost is convex piecewise linear in n, so its minimum over the narrower interval is
// still at an end or at a kink clamped into it -- split_full's candidates -- and the intersection of an
// L-natural-convex domain with a box is L-natural convex, so split_step's "n* moves by 0 or +1" holds.
// The two shortcuts hold on the narrowed interval because it is a sub-interval of the one they were argued
// for: at w = 1, 0 <= nL <= nU <= 1 still, so every kink clamps to an end and the two end tries are
// split_full's; at w = 2, [nL, nU] is inside [0, 2] still, so the tries 0, 1, 2 clamped into it visit
// every integer of it, split_full's candidates among them. (With wlo = max(1, w_min, nlo) > 1 the
// shortcuts are not taken: both fall back to split_full, as on a BoundRec.)
__device__ inline bool split_full(const BoxRec &r, int w, double &g, int &n, int s[4]) {
    return split_full_impl<false, BoxRec>(r, w, g, n, s);
}
__device__ inline bool split_full(const UBoxRec &r, int w, double &g, int &n, int s[4]) {
    return split_full_impl<true, UBoxRec>(r, w, g, n, s);
}
__device__ inline bool split_first(const BoxRec &r, int w, double &g, int &n, int s[4]) {
    return split_first_impl(r, w, g, n, s);
}
__device__ inline bool split_second(const BoxRec &r, int w, double &g, int &n, int s[4]) {
    return split_second_impl(r, w, g, n, s);
}
__device__ inline bool split_step(const BoxRec &r, int w, int n_prev, double &g, int &n, int s[4]) {
    return split_step_impl(r, w, n_prev, g, n, s);
}

// The lane's folded bounds of a boxed call: nlo = max(0, n_min_i); the link row n_i <= w_i makes
// lo_i = max(lo_i, nlo_i) an implied bound of the same MILP, used in sum lo, R and as the first table
// entry. nhi'_i = min(nhi_i, n_max_i) with nhi_i = W on a GPU device, else 0: nlo_i > W already gives
// sum lo > W (lo_i >= nlo_i, every lo >= 1), so the crossing test nlo_i > nhi'_i needs n_max and the GPU
// flag alone and is one ballot, formed once for every k.
__device__ inline bool box_fold(const Wave &sg, bool act, int gpu, int nmn, int nmx, int &lo, int &nlo) {
    nlo = min(max(0, nmn), kBoundCap);
    lo = max(lo, nlo);
    return sg.any(act && nlo > min(gpu ? 0x7fffffff : 0, nmx));
}

// The table route of the bounded sweep (route 3): fleets of any sizes 1 .. kK1MaxM under their bounds, every
// k, in one launch with the table kernel's LDS slice. What the register route leaves to the general route --
// k > 1 with room, R + 1 > kDpLanes, small fleets of a long model -- is solved here by the table machinery
// on bounded records: table_entry builds w = wlo + e and masks w > whi, the DP sees only R1 = W - sum lo + 1
// and the tables. The slice is the one plan_sweep sizes for the unbounded batch: sum lo >= M, so every
// bounded R1 fits it. No fleet is handed back (A.want = 0: no flag bytes, no hand-back flag, no scratch), and
// the waves share nothing, so launches on different streams need no ordering between them.

// Device records for table_pass: lane i holds device i's record with its bounds (M <= 64), other lanes
// fetch it by shuffle, wlo / whi with the record.
struct BoundSrc {
    using Rec = BoundRec;
    const BoundRec *me;
    __device__ inline void load(BoundRec &r, const WaveCtx &, int i) const {
        static_cast<FieldRec &>(r) = me->shfl(i);
        r.wlo = __shfl(me->wlo, i);
        r.whi = __shfl(me->whi, i);
    }
};
struct BoxSrc {  // the same for box records: nlo / nhi travel with wlo / whi
    using Rec = BoxRec;
    const BoxRec *me;
    __device__ inline void load(BoxRec &r, const WaveCtx &w, int i) const {
        BoundSrc{me}.load(r, w, i);
        r.nlo = __shfl(me->nlo, i);
        r.nhi = __shfl(me->nhi, i);
    }
};
__device__ inline BoundSrc bound_src(const BoundRec *me) { return BoundSrc{me}; }
__device__ inline BoxSrc bound_src(const BoxRec *me) { return BoxSrc{me}; }

// What a lane brings to bounded_fleet, every load issued together before the body: the fleet's extent, the
// lane's k_j / W_j, its device's fields and its bounds (no bound where an array is absent; n_min / n_max
// only with Args = BoxArgs: two more coalesced 4-byte loads beside the two w bounds and the 18 fields).
struct BoundedLane {
    int64_t d0;
    int M, kj, Wj;
    DevFields mf;
    int wmn, wmx, nmn, nmx;
};

template <class Args>
__device__ inline BoundedLane bounded_lane(const SweepArgs &A, const Args &Bd, int lane, int64_t d0, int M) {
    BoundedLane in;
    const bool kl = lane < A.n_k;
    in.kj = A.ks[kl ? lane : 0];
    in.Wj = kl ? A.Ws[lane] : 0;
    in.d0 = d0;
    in.M = M;
    const int64_t g = d0 + (lane < M ? lane : 0);
    in.mf = load_fields(A.F, g);
    in.wmn = Bd.w_min ? Bd.w_min[g] : 0;
    in.wmx = Bd.w_max ? Bd.w_max[g] : 0x7fffffff;
    in.nmn = 0;
    in.nmx = 0x7fffffff;
    if constexpr (std::is_same<Args, BoxArgs>::value) {
        in.nmn = Bd.n_min ? Bd.n_min[g] : 0;
        in.nmx = Bd.n_max ? Bd.n_max[g] : 0x7fffffff;
    }
    return in;
}

// One fleet of M <= kK1MaxM devices (lane = device) under its bounds, on either fused route. The settled
// verdicts, the objective's order of additions and every store follow sweep_fleet, so bounds that never bind
// give the sweep's bits: halda_sweep_kernel's on the register route, halda_sweep_tables_kernel's on the
// table route.
// kTables = false, the register route (M = A.uM): the host sends only batches the register sweep takes
// alone (plan_sweep's kRegAlone): every k > 1 has W < M <= sum lo, so an open instance is k = 1 with
// R = W - sum lo < kDpLanes, solved by k1_alloc and, for what the greedy does not take, k1_dp -- both exact.
// kTables = true, the table route: an open k follows the table branch of sweep_fleet<true, false> on a
// BoundRec with R = W - sum lo: k1_alloc where that branch takes it (k = 1, or R = 0 where every w_i = lo_i
// is forced), else the tables and the DP, the objective in that branch's order of additions. A.k1dp (the
// test path) sends every instance to the tables.
// Rec = BoxRec (the two box kernels): the lane's n_min / n_max too; lo is folded with nlo and the n crossing
// joins the w crossing. A leaf may then start above lo or be empty. On the register route k1_alloc hands it
// to k1_dp, which takes any leaf shape (an empty leaf: its row is all +inf, K1_INFEASIBLE). On the table
// route a leaf that starts above lo has +inf first table entries (leaf_ranges' lo > 0, the DP's usual case of
// a masked entry) and an empty leaf an all +inf row (LeafInfo.empty: dp_pass finds nothing, INFEASIBLE);
// where k1_alloc is tried first it hands either case back (K1_FALLBACK) to the tables.
template <class Rec, bool kTables>
__device__ inline void bounded_fleet(const SweepArgs &A, int f, const WaveCtx &w, const Wave &sg,
                                     const BoundedLane &in) {
    constexpr bool kBox = !std::is_same<Rec, BoundRec>::value;
    const FleetOut &O = A.out;
    const int lane = sg.sl;
    const bool kl = lane < A.n_k;
    const int kj = in.kj, Wj = in.Wj;
    const int64_t d0 = in.d0;
    const int M = in.M;
    const int outs = A.outs;
    const bool act = lane < M;
    const DevFields &mf = in.mf;
    const int wmn = in.wmn, wmx = in.wmx;
    Rec me = {};
    int bad = 0;
    static_cast<FieldRec &>(me) = field_rec(A.Mo, mf, bad);
    bad = act ? bad : 0;
    double tsum = 0.0, xsum = 0.0, kappa = 0.0;
    fleet_offsets_regs<Wave, false>(A.Mo, mf, M, sg, tsum, xsum, kappa);
    bad = sg.any(bad != 0) ? 1 : 0;
    // lo_i = max(1, w_min_i); hi_i = min(W, w_max_i). sum lo > W, some lo_i > hi_i and sum hi < W are
    // bound-infeasible. A lo_i > W already gives sum lo > W (every lo >= 1), so the crossing test needs
    // w_max alone; and where no bound crosses (every w_max_i >= lo_i >= 1) sum min(W, w_max_i) < W exactly
    // when sum w_max_i < W: all three tests are formed once, from the capped integer sums and the ballot,
    // for every k of the call.
    int lo = min(max(1, wmn), kBoundCap);
    bool ncross = false;
    if constexpr (kBox) {
        ncross = box_fold(sg, act, me.gpu, in.nmn, in.nmx, lo, me.nlo);
        me.nhi = in.nmx;
    }
    const int sumlo = sg.sum_i(act ? lo : 0);
    const int sumhi = sg.sum_i(act ? min(max(wmx, 0), kBoundCap) : 0);
    const bool cross = sg.any(act && lo > wmx) || ncross;
    double best = kInf;
    int best_k = 0;
    constexpr int kOpen = 1000;
    int stj = kOpen;
    if (!(Wj < 1000000)) stj = HALDA_STATUS_UNSUPPORTED;
    else if (sumlo > Wj) stj = HALDA_STATUS_INFEASIBLE;  // sum lb(w) > W (without bounds: M > W)
    else if (bad) stj = HALDA_STATUS_UNSUPPORTED;
    else if (cross || sumhi < Wj) stj = HALDA_STATUS_INFEASIBLE;
    if (kl && stj != kOpen) {
        const int64_t inst = int64_t(f) * A.n_k + lane;
        if (outs & kOutObk) O.obj_by_k[inst] = kInf;
        if (outs & kOutSt) O.status[inst] = stj;
    }
    if ((outs & kOutXZ) && (outs & kOutXC)) {  // x / c of a settled instance are zero
        uint64_t settled = sg.bits(kl && stj != kOpen);
        while (settled) {
            const int j = __builtin_ctzll(settled);
            settled &= settled - 1;
            zero_xc(A, O, int64_t(f) * A.n_k + j, M, lane);
        }
    }
    uint64_t todo = sg.bits(kl && stj == kOpen);
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        opaque_rec(me);
        const int k = sg.bcast(kj, j);
        const int W = sg.bcast(Wj, j);
        const int64_t inst = int64_t(f) * A.n_k + j;
        const double kc = double(k - 1);
        const int R = W - sumlo;
        int st;
        double obj = kInf;
        bool improved = false;
        int rc = K1_FALLBACK, e = 0, rounds = 0, nE = 0;
        double gE = 0.0;
        bool haveE = true;  // gE / nE hold the split at w = lo + e (k1_alloc), else split here (after k1_dp)
        me.W = W;
        me.wlo = lo;
        me.whi = min(W, wmx);
        // k = 1: the register greedy; R = 0: every w_i = lo_i is forced, so the allocation that minimises
        // sum g is the answer for any k (the output adds (k - 1) max_i H_i)
        if constexpr (kTables) {
            if ((k == 1 || R == 0) && (HALDA_SWEEP_TABLE_K1 || R == 0) && !A.k1dp)
                rc = k1_alloc(me, M, R, sg, e, rounds, gE, nE);
        } else {
            if (k == 1 || R == 0) {
                if (!A.k1dp) rc = k1_alloc(me, M, R, sg, e, rounds, gE, nE);
                if (rc == K1_FALLBACK && R < kDpLanes) {
                    rc = k1_dp(me, M, R, sg, e, w.dparg);
                    haveE = false;
                }
            }
        }
        if (rc == K1_INFEASIBLE) {
            st = HALDA_STATUS_INFEASIBLE;
        } else if (rc == K1_OK) {
            double g = 0.0, H = 0.0, z = 0.0;
            int n = 0, sl[4] = {0, 0, 0, 0};
            const int wl = lo + e;
            const bool need_h = kc != 0.0 || (outs & kOutX);
            if (act) {
                if (haveE) {
                    g = gE;
                    n = nE;
                    rec_slacks(me, wl, n, sl);
                } else {
                    split_full(me, wl, g, n, sl);
                }
                if (need_h) {
                    double P, Q;
                    dev_cycle(me, wl, n, sl, P, Q);
                    z = Q > P ? 0.5 * (Q - P) : 0.0;
                    H = Q >= P ? 0.5 * (P + Q) : P;
                }
            }
            const double hmax = need_h ? fmax(0.0, sg.max_f64(act ? H : 0.0)) : 0.0;
            obj = sg.sum_f64(act ? g : 0.0) + kc * hmax;
            obj = obj + tsum;
            obj = obj + xsum;
            obj = obj + kappa;
            st = HALDA_STATUS_OPTIMAL;
            improved = obj < best;
            if (act) {
                if (outs & kOutXC) put_xc(A, O, inst, M, lane, wl, n, sl, z, me);
                if (improved) {
                    O.w[d0 + lane] = wl;
                    O.n[d0 + lane] = n;
                }
            }
            if (lane == 0 && (outs & kOutXC)) put_xc_cycle(A, O, inst, M, hmax, kc);
        } else if constexpr (!kTables) {
            // k > 1 with room, or R + 1 > kDpLanes: not a batch the host sends here (the general route's)
            st = HALDA_STATUS_UNSUPPORTED;
        } else {
            Inst I = {};
            I.inst = int(inst);
            I.M = M;
            I.W = W;
            I.Wd = double(W);
            I.kc = kc;
            I.iC = 7 * M;
            I.R1 = R + 1;
            I.RS = odd_stride(I.R1);
            int64_t nodes = 0;
            // a guard: the host sizes the slice from the unbounded batch, which holds every bounded instance
            const bool too_large = M > A.mmax || I.R1 > A.r1max || int64_t(M) * I.RS > (kc > 0.0 ? A.tab_kc : A.tab);
            int feas = 1;
            if (!too_large) {
                table_pass<64>(bound_src(&me), w, I, lane);
                wave_sync();
                feas = dp_pass(w, I, lane, nodes) ? 1 : 0;
            }
            if (too_large) {
                st = HALDA_STATUS_TOO_LARGE;
            } else if (!feas) {
                st = HALDA_STATUS_INFEASIBLE;
            } else {
                // solution: per device (w, n, least slacks, z), sum of costs, largest cycle time
                double gs = 0.0, hmax = 0.0;
                int wl = 0, n = 0;
                if (act) {
                    wl = lo + w.st0[lane];
                    double gd = 0.0, P, Q;
                    int sl[4] = {0, 0, 0, 0};
                    split_full(me, wl, gd, n, sl);
                    dev_cycle(me, wl, n, sl, P, Q);
                    gs += gd;
                    hmax = fmax(hmax, Q >= P ? 0.5 * (P + Q) : P);
                    if (outs & kOutXC) put_xc(A, O, inst, M, lane, wl, n, sl, Q > P ? 0.5 * (Q - P) : 0.0, me);
                }
                hmax = sg.max_f64(hmax);
                obj = sg.sum_f64(gs) + kc * hmax;
                obj = obj + tsum;
                obj = obj + xsum;
                obj = obj + kappa;
                st = HALDA_STATUS_OPTIMAL;
                improved = obj < best;
                if (improved && act) {
                    O.w[d0 + lane] = wl;
                    O.n[d0 + lane] = n;
                }
                if (lane == 0 && (outs & kOutXC)) put_xc_cycle(A, O, inst, M, hmax, kc);
            }
            wave_sync();  // tables / st0 are rewritten by the next k
        }
        if (improved) {
            best = obj;
            best_k = k;
        }
        // x / c of a non-optimal instance are zero
        if ((outs & kOutXZ) && st != HALDA_STATUS_OPTIMAL) zero_xc(A, O, inst, M, lane);
        if (lane == 0) {
            if (outs & kOutObk) O.obj_by_k[inst] = st == HALDA_STATUS_OPTIMAL ? obj : kInf;
            if (outs & kOutSt) O.status[inst] = st;
        }
    }
    if (lane == 0) {
        O.best_k[f] = best_k;
        O.obj_value[f] = best;
    }
    if (best_k == 0 && act) {
        O.w[d0 + lane] = 0;
        O.n[d0 + lane] = 0;
    }
}

// The fused route's kernels -- the register sweep of a batch of fleets of one size A.uM <= kK1MaxM that needs
// no table launch (the host checks both: the sub-fleet, variants and plans kernels' gate), under per-device
// bounds. One wave per fleet, kSweepWavesPerBlock per workgroup, lane = device; the lane's bounds are 4-byte
// loads issued with the 18 field loads.
template <class Rec, class Args>
__device__ inline void bounded_regs(const SweepArgs &A, const Args &Bd) {
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    if (f >= A.F.n_fleets) return;
    const int lane = int(threadIdx.x & 63);
    const int M = A.uM;
    const int64_t base = sload_i64(A.F.dev_off);
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    bounded_fleet<Rec, false>(A, f, w, Wave(lane), bounded_lane(A, Bd, lane, base + int64_t(f) * M, M));
}

__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_bounds_kernel(
    SweepArgs A, BoundArgs Bd) {
    bounded_regs<BoundRec>(A, Bd);
}

__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_box_kernel(
    SweepArgs A, BoxArgs Bx) {
    bounded_regs<BoxRec>(A, Bx);
}

// The table route's kernels: one wave per fleet in 64-thread workgroups on a persistent grid, each with the
// table kernel's dynamic LDS slice (make_slice of the launch's shape; the same slice with the n box: folding
// nlo into lo only raises sum lo), the fleets dealt out as sweep_body deals them (workgroup b takes fleets b,
// b + grid, ...). No spin-wait and nothing shared between waves: the only synchronisation is wave_sync within
// the one wave.
template <class Rec, class Args>
__device__ inline void bounded_tables(const SweepArgs &A, const Args &Bd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const WaveCtx w = wave_ctx(smem, make_slice(A.mmax, A.r1max, A.tab, A.tab_kc));
    const int nf = A.F.n_fleets;
    for (int64_t b = blockIdx.x; b < nf; b += gridDim.x) {
        const int f = int(b);
        // the fleet's extent through the scalar cache (dev_off is read-only to the kernel)
        const int64_t d0 = A.uM > 0 ? sload_i64(A.F.dev_off) + int64_t(f) * A.uM : sload_i64(A.F.dev_off + f);
        const int M = A.uM > 0 ? A.uM : int(sload_i64(A.F.dev_off + f + 1) - d0);
        bounded_fleet<Rec, true>(A, f, w, Wave(lane), bounded_lane(A, Bd, lane, d0, M));
    }
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_bounds_tables_kernel(SweepArgs A,
                                                                                                  BoundArgs Bd) {
    bounded_tables<BoundRec>(A, Bd);
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_box_tables_kernel(SweepArgs A,
                                                                                               BoxArgs Bx) {
    bounded_tables<BoxRec>(A, Bx);
}

// ---------------------------------------------------------------- many boxes on one table
// halda_solve_fleets_boxes: one fleet table under n_box boxes in one launch. The bound arrays are box-major
// (box b's plane of array a at a + b * nd, nd = dev_off[n_fleets], device layout inside a plane) and so are
// the outputs, which is the layout of a batch of n_box * n_fleets fleets -- halda_sweep_variants_kernel's, with
// "variant" read as "box": box b's fleet f is output fleet b * n_fleets + f for best_k / obj_value / obj_by_k /
// status / x / c / x_off (bounded_fleet's fleet index), and its devices' w / n lie at b * nd + their table
// index. A wave runs bounded_fleet on the lane bounded_lane forms from the box's planes, with the lane's d0 --
// which the body uses for the w / n stores alone -- moved to the box's slice: the same code on the same fields
// and bounds as the box's own halda_solve_fleets_boxed launch, so the same bits. The record type is that call's
// choice too, made once per launch (wave-uniform): a box record when an n array was passed, else a bound record.
struct BoxesArgs {
    const int32_t *w_min, *w_max, *n_min, *n_max;  // halda_boxes: [n_box * dev_off[n_fleets]]; any may be NULL
    int n_box;
};

__device__ inline const int32_t *boxes_plane(const int32_t *a, int64_t off) { return a ? a + off : nullptr; }

template <class Rec, bool kTables>
__device__ inline void boxes_fleet(const SweepArgs &A, const BoxesArgs &Bs, int b, int f, int64_t d0, int M, int64_t nd,
                                   const WaveCtx &w, int lane) {
    const int64_t off = int64_t(b) * nd;
    BoundedLane in;
    if constexpr (std::is_same<Rec, BoxRec>::value)
        in = bounded_lane(A, BoxArgs{boxes_plane(Bs.w_min, off), boxes_plane(Bs.w_max, off), boxes_plane(Bs.n_min, off),
                                     boxes_plane(Bs.n_max, off)},
                          lane, d0, M);
    else
        in = bounded_lane(A, BoundArgs{boxes_plane(Bs.w_min, off), boxes_plane(Bs.w_max, off)}, lane, d0, M);
    in.d0 = off + d0;  // where the slice's w / n go
    bounded_fleet<Rec, kTables>(A, b * A.F.n_fleets + f, w, Wave(lane), in);
}

// The register form: bounded_regs' body, one wave per (box, fleet), blockIdx.y the box.
__global__ __launch_bounds__(64 * kSweepWavesPerBlock, HALDA_SWEEP_WAVES_PER_SIMD) void halda_sweep_boxes_kernel(
    SweepArgs A, BoxesArgs Bs) {
    const int f = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * kSweepWavesPerBlock + int(threadIdx.x >> 6));
    const int nf = A.F.n_fleets;
    if (f >= nf) return;
    const int b = int(blockIdx.y);
    const int lane = int(threadIdx.x & 63);
    const int M = A.uM;
    const int64_t base = sload_i64(A.F.dev_off), nd = sload_i64(A.F.dev_off + nf);
    __shared__ uint8_t dparg[kSweepWavesPerBlock][64 * kDpLanes];
    WaveCtx w = {};
    w.dparg = dparg[threadIdx.x >> 6];
    const int64_t d0 = base + int64_t(f) * M;
    if (Bs.n_min || Bs.n_max) boxes_fleet<BoxRec, false>(A, Bs, b, f, d0, M, nd, w, lane);
    else boxes_fleet<BoundRec, false>(A, Bs, b, f, d0, M, nd, w, lane);
}

// The table form: bounded_tables' persistent loop over the n_box * n_fleets (box, fleet) items, box-major, on
// the one LDS slice (it depends on the unbounded shape only, so it serves every box).
template <class Rec>
__device__ inline void boxes_tables(const SweepArgs &A, const BoxesArgs &Bs, unsigned char *smem) {
    const int lane = threadIdx.x;
    const WaveCtx w = wave_ctx(smem, make_slice(A.mmax, A.r1max, A.tab, A.tab_kc));
    const int nf = A.F.n_fleets;
    const int64_t nd = sload_i64(A.F.dev_off + nf), items = int64_t(Bs.n_box) * nf;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int b = int(it / nf), f = int(it - int64_t(b) * nf);
        const int64_t d0 = A.uM > 0 ? sload_i64(A.F.dev_off) + int64_t(f) * A.uM : sload_i64(A.F.dev_off + f);
        const int M = A.uM > 0 ? A.uM : int(sload_i64(A.F.dev_off + f + 1) - d0);
        boxes_fleet<Rec, true>(A, Bs, b, f, d0, M, nd, w, lane);
    }
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_boxes_tables_kernel(SweepArgs A,
                                                                                                 BoxesArgs Bs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (Bs.n_min || Bs.n_max) boxes_tables<BoxRec>(A, Bs, smem);
    else boxes_tables<BoundRec>(A, Bs, smem);
}

// ---------------------------------------------------------------- total move budget (halda_solve_fleets_budget)
// The fixed-k problem at the incumbent's k with sum_i |w_i - w0_i| <= B added: the constraint couples the
// devices, so it is not a narrowing of column bounds. Both plans sum to W, hence sum |delta| = 2 sum delta+;
// the solver works in p = sum_i max(0, w_i - w0_i) with P = B / 2 and answers every budget p = 0 .. P at once.
// Only w_i in [w0_i - P, w0_i + P] can matter: the tables G / H are built on that window by table_pass
// (rows of at most 2 P + 1 entries), and the frontier DP below carries the layers released and loaded so far
// (both end at p). k > 1 scans the cycle-time thresholds T pass by pass (DESIGN.md section 2's exact scan in
// its pass-per-candidate form: nothing is assumed of the rows' shape).
struct BudgetArgs {
    const int32_t *w0, *w_min, *w_max;  // device layout; w_min / w_max may be NULL
    int P;                              // halda_budget.max_p
    int64_t nd;                         // devices of the table: the stride of the w / n planes
    int32_t *status;                    // [fleet][P + 1]
    double *obj;                        // [fleet][P + 1]
    int32_t *moved;                     // [fleet][P + 1]
    int32_t *w, *n;                     // [P + 1][nd]
};

// ---------------------------------------------------------------- a changed fleet (halda_solve_change)
// Re-placement after a device is lost or joins. An item is a sub-fleet of a parent fleet (SubArgs: the listed
// devices in list order) with the layers each listed device holds now, w0_i >= 0 (0: a joiner). The deficit
// D = W - sum w0 >= 0 is what the lost devices held. With delta_i = w_i - w0_i, loaded = sum max(0, delta)
// and released = sum max(0, -delta), every plan has loaded = D + released; point p of the frontier is the
// optimum of the list's fixed-k problem over the plans with released <= p. Only w_i in
// [w0_i - P, w0_i + D + P] can matter: G / H are built on that window by table_pass (rows of at most
// 2 P + D + 1 entries), and the frontier DP below carries the state (r, l): r the layers released so far,
// in [0, P], l the layers loaded so far, in [0, D + P]. The exact-p answers are the final states (p, D + p).
// With D = 0 and every w0_i >= 1 this is the budget problem, solved by the same body: hence its bits.
struct ChangeArgs {
    SubArgs S;                          // the items; A.F is the parent table with n_fleets = the item count
    const int32_t *w0, *w_min, *w_max;  // laid out by sub_off; w_min / w_max may be NULL
    int P, Dmax;                        // halda_change.max_p / max_deficit
    int64_t nd;                         // sub_off[n_items]: the stride of the w / n planes
    int32_t *status;                    // [item][P + 1]
    double *obj;                        // [item][P + 1]
    int32_t *loaded, *released;         // [item][P + 1]
    int32_t *w, *n;                     // [P + 1][nd]
};

// ---------------------------------------------------------------- the frontier body of both kernels
// Both problems are one: devices that hold w0_i layers, a deficit D >= 0 of layers nobody holds (0 under a
// move budget), and per point p the best plan that releases at most p layers (and so loads at most D + p).
// frontier_item solves one fleet or item; a job (BudgetJob, ChangeJob) supplies where a lane's device and
// inputs are read, the incumbent rule and the deficit, how a state is laid out in the value plane, and the
// integers a point reports. The two kernels differ in nothing else.
//
// The wave's LDS slice (bytes): G and, for k > 1, H as mmax rows of RS doubles (RS odd); two value planes of
// S doubles; one arg-min byte plane of S per device; per device wlo - w0; per point the plan's table indices
// (bytes) and its n (ints).
struct FrontierSlice {
    int64_t G, H, V, arg, off, plan, nplan, total;
    int S, RS;
};

__host__ __device__ inline FrontierSlice frontier_slice(int mmax, int P, int RS, int S, bool kc) {
    FrontierSlice s;
    s.RS = RS;
    s.S = S;
    int64_t o = 0;
    s.G = o;     o = align16(o + int64_t(mmax) * s.RS * 8);
    s.H = o;     o = align16(o + (kc ? int64_t(mmax) * s.RS * 8 : 0));
    s.V = o;     o = align16(o + 2 * int64_t(s.S) * 8);
    s.arg = o;   o = align16(o + int64_t(mmax) * s.S);
    s.off = o;   o = align16(o + int64_t(mmax) * 4);
    s.plan = o;  o = align16(o + int64_t(P + 1) * mmax);
    s.nplan = o; o = align16(o + int64_t(P + 1) * mmax * 4);
    s.total = o;
    return s;
}

// The budget kernel's: rows of 2 P + 1 entries, S = (2 P + 1)(P + 1) states (BudgetMap).
__host__ __device__ inline FrontierSlice budget_slice(int mmax, int P, bool kc) {
    return frontier_slice(mmax, P, 2 * P + 1, (2 * P + 1) * (P + 1), kc);
}

// The change kernel's: rows of (2 P + Dmax + 1) | 1 entries, S = (P + 1)(Dmax + P + 1) states (ChangeMap).
__host__ __device__ inline FrontierSlice change_slice(int mmax, int P, int Dmax, bool kc) {
    return frontier_slice(mmax, P, (2 * P + Dmax + 1) | 1, (P + 1) * (Dmax + P + 1), kc);
}

struct FrontierCtx {
    double *V;       // two planes of S
    uint8_t *arg;    // [device][S]
    int *off;        // [device] wlo - w0
    uint8_t *plan;   // [point][mmax]
    int *nplan;      // [point][mmax]
    int S, RS, P, mmax;
};

// The kernels' slice binding: w.G / w.H and the frontier's own regions.
__device__ inline FrontierCtx frontier_ctx(unsigned char *smem, const FrontierSlice &sl, int P, int mmax, WaveCtx &w) {
    w.G = reinterpret_cast<double *>(smem + sl.G);
    w.H = reinterpret_cast<double *>(smem + sl.H);
    FrontierCtx c;
    c.V = reinterpret_cast<double *>(smem + sl.V);
    c.arg = smem + sl.arg;
    c.off = reinterpret_cast<int *>(smem + sl.off);
    c.plan = smem + sl.plan;
    c.nplan = reinterpret_cast<int *>(smem + sl.nplan);
    c.S = sl.S;
    c.RS = sl.RS;
    c.P = P;
    c.mmax = mmax;
    return c;
}

constexpr uint8_t kFrontierNone = 255;  // arg-min of a state no transition reaches (an entry is at most 254)

// How a state (r released, l loaded) lies in a value plane. The budget kernel's plane is indexed by the net
// deviation l - r in [-P, P] and l in [0, P]: of its (2 P + 1)(P + 1) slots those with r outside [0, P] hold
// no state. (Its slice, and with it the gate and the occupancy, rest on that plane.)
struct BudgetMap {
    int P, P1;
    __device__ int count() const { return (2 * P + 1) * P1; }
    __device__ bool decode(int s, int &r, int &l) const {
        const int dq = s / P1;
        l = s - dq * P1;
        r = l - (dq - P);
        return r >= 0 && r <= P;
    }
    __device__ int at(int r, int l) const { return (l - r + P) * P1 + l; }
    __device__ int start() const { return P * P1; }
    __device__ int final(int p) const { return P * P1 + p; }
};

// The change kernel's plane: r in [0, P] by l in [0, D + P], LQ = D + P + 1 the item's own row length
// (LQ (P + 1) <= S). Every slot is a state.
struct ChangeMap {
    int P, LQ, D;
    __device__ int count() const { return (P + 1) * LQ; }
    __device__ bool decode(int s, int &r, int &l) const {
        r = s / LQ;
        l = s - r * LQ;
        return true;
    }
    __device__ int at(int r, int l) const { return r * LQ + l; }
    __device__ int start() const { return 0; }
    __device__ int final(int p) const { return p * LQ + D + p; }
};

// One DP over the M devices with the entries H > T masked (kc == 0: no mask). Lanes own states; a transition
// tries the device's R1 entries in ascending order and keeps the first least value (strict "<": the least
// w_i). Returns the plane that holds the values after the last device; arg holds every device's arg-min plane.
template <class Map>
__device__ inline const double *frontier_dp(const WaveCtx &w, const FrontierCtx &c, const Map &m, int M, int R1,
                                            double kc, double T, int lane) {
    const int Sn = m.count(), s0 = m.start();
    double *cur = c.V, *nxt = c.V + c.S;
    for (int s = lane; s < Sn; s += 64) cur[s] = s == s0 ? 0.0 : kInf;
    wave_sync();
    for (int i = 0; i < M; ++i) {
        const int oi = c.off[i];
        const double *Gi = w.G + i * c.RS, *Hi = w.H + i * c.RS;
        uint8_t *ai = c.arg + int64_t(i) * c.S;
        for (int s = lane; s < Sn; s += 64) {
            int r, l;
            double best = kInf;
            int be = kFrontierNone;
            if (m.decode(s, r, l)) {
                for (int e = 0; e < R1; ++e) {
                    const int delta = oi + e;
                    const int lp = l - max(0, delta), rp = r - max(0, -delta);
                    if (lp < 0 || rp < 0) continue;
                    if (kc > 0.0 && !(Hi[e] <= T)) continue;
                    const double v = cur[m.at(rp, lp)] + Gi[e];
                    if (v < best) {
                        best = v;
                        be = e;
                    }
                }
            }
            nxt[s] = best;
            ai[s] = uint8_t(be);
        }
        wave_sync();
        double *t = cur;
        cur = nxt;
        nxt = t;
    }
    return cur;
}

// The plan of point p (lane p) with a finite final value: from state (p, D + p) after the last device back
// to (0, 0). Every state on that path has a finite value, so its arg-min is an entry of the row and the
// predecessor it names is a valid state.
template <class Map>
__device__ inline void frontier_backtrack(const FrontierCtx &c, const Map &m, int M, int D, int p) {
    int r = p, l = D + p;
    for (int i = M - 1; i >= 0; --i) {
        const int e = c.arg[int64_t(i) * c.S + m.at(r, l)];
        c.plan[p * c.mmax + i] = uint8_t(e);
        const int delta = c.off[i] + e;
        l -= max(0, delta);
        r -= max(0, -delta);
    }
}

// What a lane of an item reads and writes: the item's length, its device in the table, its entry of w0 /
// w_min / w_max and its entry of a w / n plane (lanes past M read the first device's and write nothing).
struct FrontierLane {
    int M;
    int64_t dev, in, out;
};

// A move budget: item f is fleet f of the table, every array in device layout; the incumbent is a plan
// (w0_i >= 1, sum w0 = W), so nothing is orphaned; a point reports moved = sum |w - w0|.
struct BudgetJob {
    using Args = BudgetArgs;
    using Map = BudgetMap;
    __device__ static FrontierLane lane_of(const SweepArgs &A, const Args &, int f, int lane) {
        // the fleet's extent through the scalar cache (dev_off is read-only to the kernel)
        const int64_t d0 = A.uM > 0 ? sload_i64(A.F.dev_off) + int64_t(f) * A.uM : sload_i64(A.F.dev_off + f);
        const int M = A.uM > 0 ? A.uM : int(sload_i64(A.F.dev_off + f + 1) - d0);
        const int64_t g0 = d0 + (lane < M ? lane : 0);
        return {M, g0, g0, d0 + lane};
    }
    __device__ static bool bad_w0(const Args &, const Wave &sg, bool act, int w0, int sumw0, int W) {
        return sg.any(act && w0 < 1) || sumw0 != W;
    }
    __device__ static int deficit(bool, int, int) { return 0; }
    __device__ static Map map(int P, int) { return {P, P + 1}; }
    __device__ static int count(int w0, int wl) { return abs(wl - w0); }
    __device__ static void report(const Args &J, int64_t at, bool, int, int moved) { J.moved[at] = moved; }
};

// A changed fleet: item `it` lists devices of its parent (lane j gathers the j-th: halda_sweep_subfleets_kernel's
// index read), every array laid out by sub_off; w0_i >= 0 and the deficit D = W - sum w0 in [0, Dmax]; a point
// reports released = sum max(0, w0 - w) and loaded = D + released.
struct ChangeJob {
    using Args = ChangeArgs;
    using Map = ChangeMap;
    __device__ static FrontierLane lane_of(const SweepArgs &A, const Args &J, int it, int lane) {
        // the item's extent, parent and the parent's first device: wave-uniform reads through the scalar cache
        const int64_t so = sload_i64(J.S.sub_off + it);
        const int M = A.uM > 0 ? A.uM : int(sload_i64(J.S.sub_off + it + 1) - so);
        const int64_t base = sload_i64(A.F.dev_off + sload_i32(J.S.parent + it));
        const int64_t o0 = so + (lane < M ? lane : 0);
        return {M, base + J.S.sub_idx[o0], o0, so + lane};
    }
    __device__ static bool bad_w0(const Args &J, const Wave &sg, bool act, int w0, int sumw0, int W) {
        return sg.any(act && w0 < 0) || sumw0 > W || W - sumw0 > J.Dmax;
    }
    // 0 where the incumbent is rejected, so that nothing is formed from it
    __device__ static int deficit(bool w0bad, int W, int sumw0) { return w0bad ? 0 : W - sumw0; }
    __device__ static Map map(int P, int D) { return {P, D + P + 1, D}; }
    __device__ static int count(int w0, int wl) { return max(0, w0 - wl); }
    __device__ static void report(const Args &J, int64_t at, bool plan, int D, int released) {
        J.loaded[at] = plan ? D + released : 0;
        J.released[at] = released;
    }
};

template <class Job>
__device__ inline void frontier_item(const SweepArgs &A, const typename Job::Args &J, int it, const WaveCtx &w,
                                     const FrontierCtx &c, const Wave &sg) {
    const int lane = sg.sl;
    const int P = J.P, P1 = P + 1;
    const int k = A.ks[0], W = A.Ws[0];
    const FrontierLane at = Job::lane_of(A, J, it, lane);
    const int M = at.M;
    const bool act = lane < M;
    const bool pt = lane < P1;
    const int wmn = J.w_min ? J.w_min[at.in] : 0;
    const int wmx = J.w_max ? J.w_max[at.in] : 0x7fffffff;
    const int w0 = min(max(J.w0[at.in], -kBoundCap), kBoundCap);
    const DevFields mf = load_fields(A.F, at.dev);
    BoundRec me = {};
    int bad = 0;
    static_cast<FieldRec &>(me) = field_rec(A.Mo, mf, bad);
    bad = act ? bad : 0;
    double tsum = 0.0, xsum = 0.0, kappa = 0.0;
    fleet_offsets_regs<Wave, false>(A.Mo, mf, M, sg, tsum, xsum, kappa);
    bad = sg.any(bad != 0) ? 1 : 0;
    const int lo = min(max(1, wmn), kBoundCap);
    const int sumlo = sg.sum_i(act ? lo : 0);
    const int sumw0 = sg.sum_i(act ? w0 : 0);
    const bool w0bad = Job::bad_w0(J, sg, act, w0, sumw0, W);  // the host entries reject it before the launch
    const int D = Job::deficit(w0bad, W, sumw0);
    // the window: a device gives up at most P layers and takes at most D + P
    const int wlo = max(lo, w0 - P), whi = min(min(W, wmx), w0 + D + P);
    const int sumwlo = sg.sum_i(act ? min(wlo, kBoundCap) : 0);
    constexpr int kOpen = 1000;
    int st = kOpen;
    if (!(W < 1000000)) st = HALDA_STATUS_UNSUPPORTED;
    else if (sumlo > W) st = HALDA_STATUS_INFEASIBLE;
    else if (bad || w0bad) st = HALDA_STATUS_UNSUPPORTED;
    else if (sumwlo > W) st = HALDA_STATUS_INFEASIBLE;  // the window cannot reach the box
    const int64_t fo = int64_t(it) * P1;
    if (st != kOpen) {
        if (pt) {
            J.status[fo + lane] = st;
            J.obj[fo + lane] = kInf;
            Job::report(J, fo + lane, false, 0, 0);
        }
        if (act)
            for (int p = 0; p < P1; ++p) {
                J.w[int64_t(p) * J.nd + at.out] = 0;
                J.n[int64_t(p) * J.nd + at.out] = 0;
            }
        return;
    }
    opaque_rec(me);
    const double kc = double(k - 1);
    me.W = W;
    me.wlo = wlo;
    me.whi = whi;
    if (act) c.off[lane] = wlo - w0;
    Inst I = {};
    I.inst = it;
    I.M = M;
    I.W = W;
    I.Wd = double(W);
    I.kc = kc;
    I.iC = 7 * M;
    I.R1 = min(W - sumwlo, 2 * P + D) + 1;
    I.RS = c.RS;
    const int R1 = I.R1;
    const typename Job::Map m = Job::map(P, D);
    table_pass<64>(bound_src(&me), w, I, lane);
    wave_sync();
    // best[p] (lane p): the least (k - 1) T + F^T_M[final state of p] and the T that gave it
    double best = kInf, bT = kInf;
    if (kc == 0.0) {
        const double *F = frontier_dp(w, c, m, M, R1, 0.0, kInf, lane);
        if (pt) best = F[m.final(lane)];
        wave_sync();
        if (pt && best < kInf) frontier_backtrack(c, m, M, D, lane);
    } else {
        const double *F = frontier_dp(w, c, m, M, R1, 0.0, kInf, lane);
        const double sinf = pt ? F[m.final(lane)] : kInf;
        // the first threshold that leaves every device an entry: max_i min_e H_i[e]
        double hmin = kInf;
        if (act)
            for (int e = 0; e < R1; ++e) hmin = fmin(hmin, w.H[lane * c.RS + e]);
        double T = sg.max_f64(act ? hmin : 0.0);
        while (T < kInf) {
            // point p is closed once (k - 1) T + S_inf[p] >= best[p]; the scan stops when every point is
            if (!sg.any(pt && !(kc * T + sinf >= best))) break;
            wave_sync();
            F = frontier_dp(w, c, m, M, R1, kc, T, lane);
            if (pt) {
                const double v = kc * T + F[m.final(lane)];
                if (v < best) {  // strict: the earliest T wins
                    best = v;
                    bT = T;
                }
            }
            double nx = kInf;  // the next distinct finite H above T
            for (int t = lane; t < M * R1; t += 64) {
                const int i = t / R1, e = t - i * R1;
                const double h = w.H[i * c.RS + e];
                if (h > T) nx = fmin(nx, h);
            }
            T = sg.min_f64(nx);
        }
        // the arg-min planes of each distinct winning T, once, for the points it won
        bool left = pt && best < kInf;
        while (sg.any(left)) {
            const double Tw = sg.min_f64(left ? bT : kInf);
            wave_sync();
            frontier_dp(w, c, m, M, R1, kc, Tw, lane);
            if (left && bT == Tw) {
                frontier_backtrack(c, m, M, D, lane);
                left = false;
            }
        }
    }
    wave_sync();
    // price every exact-p plan lane-per-device, the constants added in sweep_fleet's order
    double objv = kInf;
    int cntv = 0;
    for (int p = 0; p < P1; ++p) {
        if (!(sg.bcast(best, p) < kInf)) continue;
        double gd = 0.0, H = 0.0;
        int wl = 0, n = 0;
        if (act) {
            wl = wlo + c.plan[p * c.mmax + lane];
            double Pc, Qc;
            int sl[4] = {0, 0, 0, 0};
            split_full(me, wl, gd, n, sl);
            dev_cycle(me, wl, n, sl, Pc, Qc);
            H = fmax(0.0, Qc >= Pc ? 0.5 * (Pc + Qc) : Pc);
            c.nplan[p * c.mmax + lane] = n;
        }
        const double hmax = sg.max_f64(act ? H : 0.0);
        double obj = sg.sum_f64(act ? gd : 0.0) + kc * hmax;
        obj = obj + tsum;
        obj = obj + xsum;
        obj = obj + kappa;
        const int cnt = sg.sum_i(act ? Job::count(w0, wl) : 0);
        if (lane == p) {
            objv = obj;
            cntv = cnt;
        }
    }
    wave_sync();
    // point p: the best exact point p' <= p, the fewest layers moved (released) among equal objectives (strict
    // "<", ascending)
    double run = kInf;
    int src = -1, runcnt = 0;
    for (int p = 0; p < P1; ++p) {
        const double o = sg.bcast(objv, p);
        const int cnt = sg.bcast(cntv, p);
        if (lane >= p && o < run) {
            run = o;
            src = p;
            runcnt = cnt;
        }
    }
    if (pt) {
        J.status[fo + lane] = src >= 0 ? HALDA_STATUS_OPTIMAL : HALDA_STATUS_INFEASIBLE;
        J.obj[fo + lane] = run;
        Job::report(J, fo + lane, src >= 0, D, runcnt);
    }
    for (int p = 0; p < P1; ++p) {
        const int sp = sg.bcast(src, p);
        if (act) {
            J.w[int64_t(p) * J.nd + at.out] = sp >= 0 ? wlo + c.plan[sp * c.mmax + lane] : 0;
            J.n[int64_t(p) * J.nd + at.out] = sp >= 0 ? c.nplan[sp * c.mmax + lane] : 0;
        }
    }
    wave_sync();  // the slice is rewritten by the wave's next item
}

// halda_sweep_budget_kernel / halda_sweep_change_kernel: one wave per fleet (item) in 64-thread workgroups on a
// persistent grid, each with its dynamic LDS slice (budget_slice / change_slice of the launch's shape);
// workgroup b takes items b, b + grid, .... No spin-wait, no atomics and nothing shared between waves: the
// only synchronisation is wave_sync within the one wave.
__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_budget_kernel(SweepArgs A,
                                                                                           BudgetArgs Bg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    WaveCtx w = {};
    const FrontierCtx c = frontier_ctx(smem, budget_slice(A.mmax, Bg.P, A.ks[0] > 1), Bg.P, A.mmax, w);
    const int nf = A.F.n_fleets;
    for (int64_t f = blockIdx.x; f < nf; f += gridDim.x) frontier_item<BudgetJob>(A, Bg, int(f), w, c, Wave(lane));
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_change_kernel(SweepArgs A,
                                                                                           ChangeArgs Cg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    WaveCtx w = {};
    const FrontierCtx c = frontier_ctx(smem, change_slice(A.mmax, Cg.P, Cg.Dmax, A.ks[0] > 1), Cg.P, A.mmax, w);
    const int n = A.F.n_fleets;
    for (int64_t it = blockIdx.x; it < n; it += gridDim.x) frontier_item<ChangeJob>(A, Cg, int(it), w, c, Wave(lane));
}

// ---------------------------------------------------------------- scale-in / scale-out (halda_solve_change_subsets)
// Which devices to drop (or, from a pool, to add) under a released-layer budget: the candidates are
// halda_solve_subsets' (SubsetFleet / SubsetArgs, one combo per candidate, the same enumeration order), a
// candidate's value at point p is what halda_sweep_change_kernel writes for its list with w0 restricted to it.
// Per (d, chunk): halda_change_subsets_index_kernel writes the chunk's candidates as change items in context
// scratch, the unedited change kernel runs on them, and halda_change_subsets_pick_kernel folds the chunk into
// the frontier grid [fleet][d - min_drop][p]. No atomics, no spin-waits, nothing shared between workgroups.
struct ChangeSubsetsSrc {
    const int64_t *dev_off;             // the table's
    const int32_t *w0, *w_min, *w_max;  // per parent device, laid out by dev_off; w_min / w_max may be NULL
};

struct ChangeSubsetsItems {
    int32_t *parent;             // [n]
    int64_t *sub_off;            // [n + 1]
    int32_t *sub_idx;            // [listed devices of the launch]
    int32_t *w0, *w_min, *w_max; // the same layout (w_min / w_max unused where the source has none)
};

// One wave per candidate: the item as halda_subsets_index_kernel writes it, and beside it the kept devices'
// w0 / w_min / w_max gathered from the per-parent-device arrays (lane j: the j-th kept device).
__global__ __launch_bounds__(256) void halda_change_subsets_index_kernel(SubsetArgs U, ChangeSubsetsSrc G,
                                                                         ChangeSubsetsItems O) {
    const int i = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * 4 + int(threadIdx.x >> 6));
    if (i >= U.n) return;
    const int lane = int(threadIdx.x & 63);
    const int64_t g = U.i0 + i;
    int lo = 0, hi = U.n_fleets - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sload_i64(&U.fl[mid].item_off) <= g) lo = mid;
        else hi = mid - 1;
    }
    const SubsetFleet sf = subset_fleet(U, lo);
    const int64_t cand = g - sf.item_off;
    const uint64_t combo = sload_u64(U.combos + sf.combo_off + cand);
    const int64_t base = sload_i64(G.dev_off + lo);
    int nk;
    const int idx = subset_kept_index(sf.drop_mask, combo, sf.M, lane, &nk);
    const int64_t so = sf.list_off + cand * int64_t(sf.M - U.d) - U.l0;
    if (lane < nk) {
        O.sub_idx[so + lane] = idx;
        O.w0[so + lane] = G.w0[base + idx];
        if (G.w_min) O.w_min[so + lane] = G.w_min[base + idx];
        if (G.w_max) O.w_max[so + lane] = G.w_max[base + idx];
    }
    if (lane == 0) {
        O.parent[i] = lo;
        O.sub_off[i] = so;
        if (i == U.n - 1) O.sub_off[i + 1] = so + nk;
    }
}

struct ChangeSubsetsChunk {  // one launch's halda_change_frontier in context scratch
    const double *obj;                 // [n][P1]
    const int32_t *loaded, *released;  // [n][P1]
    const int32_t *w, *n;              // [P1][nd]
    int64_t nd;
    int32_t P1, D1, d0;                // points per item; the grid's d rows and its first d (min_drop)
};

struct ChangeSubsetGrid {  // halda_change_subset_frontier
    int32_t *status;
    double *obj;
    uint64_t *dropped_mask;
    int32_t *loaded, *released;
    int32_t *w, *n;
};

// One workgroup per fleet, for the launch's d: per point p the arg-min of the launch's items of the fleet's
// group on (raw obj, candidate index), lexicographic with strict <, as halda_subsets_pick_kernel takes it
// -- per thread over its candidates in ascending order, a wave reduction, the four waves' results through
// LDS behind ONE workgroup barrier (every p at once). Then wave v takes the points v, v + 4, ...: a cell
// whose group began in an earlier launch moves only for a strictly lower value; lane j writes parent device
// j's entry of the winner's point-p plan, read from the chunk's planes at the device's rank among the kept
// (0 for a dropped device). A group without candidates, or a cell whose candidates all have no plan at p,
// reads INFEASIBLE, +inf, mask 0, zero counts and a zero plan.
__global__ __launch_bounds__(256) void halda_change_subsets_pick_kernel(SubsetArgs U, ChangeSubsetsChunk C,
                                                                        ChangeSubsetGrid R) {
    const int f = int(blockIdx.x);
    const SubsetFleet sf = subset_fleet(U, f);
    const int lane = int(threadIdx.x & 63), wv = int(threadIdx.x >> 6);
    const int P1 = C.P1;
    const int64_t at = (int64_t(f) * C.D1 + (U.d - C.d0)) * P1;
    if (sf.cnt == 0) {
        if (U.i0 == 0)
            for (int p = wv; p < P1; p += 4) {
                if (lane == 0) {
                    R.status[at + p] = HALDA_STATUS_INFEASIBLE;
                    R.obj[at + p] = kInf;
                    R.dropped_mask[at + p] = 0;
                    R.loaded[at + p] = 0;
                    R.released[at + p] = 0;
                }
                R.w[(at + p) * 64 + lane] = 0;
                R.n[(at + p) * 64 + lane] = 0;
            }
        return;
    }
    const int64_t a = sf.item_off > U.i0 ? sf.item_off : U.i0;
    const int64_t e = sf.item_off + sf.cnt, lim = U.i0 + U.n;
    const int64_t b = e < lim ? e : lim;
    if (a >= b) return;
    __shared__ double so[4][64];
    __shared__ int64_t sc[4][64];
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
    const uint64_t below = (uint64_t(1) << lane) - 1;
    const uint64_t all = sf.M >= 64 ? ~uint64_t(0) : (uint64_t(1) << sf.M) - 1;
    for (int p = wv; p < P1; p += 4) {
        double o = so[0][p];
        int64_t c = sc[0][p];
        for (int v = 1; v < 4; ++v) subset_min(o, c, so[v][p], sc[v][p]);
        if (!first && !(o < R.obj[at + p])) continue;  // the group began earlier: only a strictly lower value moves it
        const bool ok = o < kInf;
        const uint64_t combo = U.combos[sf.combo_off + c];
        const int slot = __popcll(sf.drop_mask & below);
        const bool kept = lane < sf.M && !(((sf.drop_mask >> lane) & 1) && ((combo >> slot) & 1));
        const uint64_t km = __ballot(kept);
        const int64_t src = int64_t(p) * C.nd + sf.list_off + c * int64_t(sf.M - U.d) - U.l0 + __popcll(km & below);
        int wl = 0, nl = 0;
        if (ok && kept) {
            wl = C.w[src];
            nl = C.n[src];
        }
        R.w[(at + p) * 64 + lane] = wl;
        R.n[(at + p) * 64 + lane] = nl;
        if (lane == 0) {
            const int64_t it = (sf.item_off + c - U.i0) * P1 + p;
            R.status[at + p] = ok ? HALDA_STATUS_OPTIMAL : HALDA_STATUS_INFEASIBLE;
            R.obj[at + p] = o;
            R.dropped_mask[at + p] = ok ? ~km & all : 0;
            R.loaded[at + p] = ok ? C.loaded[it] : 0;
            R.released[at + p] = ok ? C.released[it] : 0;
        }
    }
}

// ---------------------------------------------------------------- resident single-fleet solver
// halda_resident_kernel: ONE wave that stays resident between single-fleet calls (halda_solve's
// latency path through halda_solve_fleets_host): the host writes the call's sweep arguments and the
// fleet's table into fine-grained pinned memory and bumps `seq`; the wave, polling `seq` across PCIe,
// copies the arguments into LDS, solves the fleet exactly as the per-call register launch does (the
// same sweep_fleet on the same fields, x / c included) writing into the pinned results, and publishes
// `ack` = seq with a system-scope release. No launch and no completion event per call. It leaves when
// the host sets `stop` or after `idle_ticks` of the 100 MHz real-time clock without a request (every
// wave exits: the host relaunches it on its next call), so it never outlives its process by more
// than that. All its stores are vector stores.
struct ResidentBox {
    uint32_t seq;  // host: request number, written after the request
    uint32_t pad0[15];
    uint32_t ack;  // device: the last request done
    uint32_t pad1[15];
    uint32_t stop;  // host: 1 = leave now
    uint32_t pad2[15];
    SweepArgs req;  // host: the request's sweep arguments (one fleet, a register-only plan)
};

struct ResidentArgs {
    ResidentBox *box;
    uint32_t last;        // the request number already answered
    uint32_t idle_ticks;  // s_memrealtime ticks (100 MHz) without a request before the wave leaves
};

__device__ inline uint32_t sys_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(64) void halda_resident_kernel(ResidentArgs R) {
    __shared__ SweepArgs As;
    __shared__ uint8_t dparg[64 * kDpLanes];
    const int lane = int(threadIdx.x);
    WaveCtx w = {};
    w.dparg = dparg;
    const Wave wv(lane);
    uint32_t last = R.last;
    uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (true) {
        const uint32_t stop = sys_load(&R.box->stop);
        const uint32_t seq = sys_load(&R.box->seq);
        if (stop) break;
        if (seq == last) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > R.idle_ticks) break;
            __builtin_amdgcn_s_sleep(2);
            continue;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // the request and table written before seq
        // the sweep arguments into LDS by vector loads (nothing of the request is read through the
        // scalar cache, which does not see the host's writes)
        constexpr int kWords = int(sizeof(SweepArgs) / 4);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&R.box->req);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&As);
        for (int i = lane; i < kWords; i += 64) dst[i] = sys_load(src + i);
        __builtin_amdgcn_s_waitcnt(0);
        wave_sync();
        SweepPre pre;
        const bool kl = lane < As.n_k;
        pre.kj = As.ks[kl ? lane : 0];
        pre.Wj = kl ? As.Ws[lane] : 0;
        pre.d0 = 0;
        const int M = As.uM;
        pre.mf = load_fields(As.F, lane < M ? lane : 0);
        sweep_fleet<false, false, Wave, true, true, true>(As, As.F, As.out, 0, w, wv, &pre);
        // every result store before ack (system-scope release: the host reads them after it)
        if (lane == 0) __hip_atomic_store(&R.box->ack, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        last = seq;
        t0 = __builtin_amdgcn_s_memrealtime();
        wave_sync();
    }
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_tables_kernel(SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sweep_body<true, false>(A, batch_of(A), smem);
}

// halda_sweep_tables_variants_kernel: the table form of a variants launch (a small batch whose one launch
// is halda_sweep_tables_kernel) -- grid (the table kernel's own, n_var), every workgroup the table
// kernel's loop over the fleets with its variant's model. The host sends A.uM = 0, so sweep_fleet takes a
// fleet's extent from dev_off alone; the wave's view of dev_off is moved back by the variant's fleet offset
// v * n_fleets, so that the output fleet index sweep_fleet is handed addresses the fleet's own entry, and
// its view of w / n forward by v * dev_off[n_fleets].
__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_tables_variants_kernel(SweepArgs A,
                                                                                                       VarArgs V) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int v = int(blockIdx.y), nf = A.F.n_fleets;
    const int64_t nd = sload_i64(A.F.dev_off + nf);
    const SweepModel Mo = var_model(V, v);
    halda_fleets F = A.F;
    F.dev_off -= int64_t(v) * nf;
    FleetOut O = A.out;
    O.w += int64_t(v) * nd;
    O.n += int64_t(v) * nd;
    sweep_body<true, false>(A, SweepBatch{F, O, nullptr}, smem, Mo, v * nf);
}

__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_big_kernel(SweepArgs A) {
    sweep_body<true, true>(A, batch_of(A), A.gtab + int64_t(blockIdx.x) * A.gstride);
}

// halda_sweep_seg_kernel: fleets of at most kSegLanes devices (C2: 16) with at most kSegLanes
// k-candidates, 64 / kSegLanes fleets per wave, one per lane segment, each with an LDS slice of only
// what the lane-parallel path touches: G and H (k > 1 tables, row stride RS) and st0. Every wave
// reduction of the one-fleet-per-wave path becomes a segment butterfly (same order of additions:
// the wave butterfly's first two steps only add zeros for M <= 16), so the results are the same
// bits; what the segment path does not take is flagged for the gated halda_sweep_tables_kernel.
constexpr int kSegLanes = 16;

__host__ __device__ inline int64_t seg_slice_bytes(int mmax, int tab_kc) {
    return 2 * align16(int64_t(tab_kc) * 8) + align16(int64_t(mmax) * 4);
}

#ifndef HALDA_SEG_WAVES_PER_SIMD
#define HALDA_SEG_WAVES_PER_SIMD 2
#endif

__global__ __launch_bounds__(64, HALDA_SEG_WAVES_PER_SIMD) void halda_sweep_seg_kernel(SweepArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kPer = 64 / kSegLanes;
    const int lane = threadIdx.x;
    const Seg<kSegLanes> sg(lane);
    const int seg = lane / kSegLanes;
    const int64_t tb = align16(int64_t(A.tab_kc) * 8);
    unsigned char *base = smem + int64_t(seg) * seg_slice_bytes(A.mmax, A.tab_kc);
    WaveCtx w = {};
    w.G = reinterpret_cast<double *>(base);
    w.H = reinterpret_cast<double *>(base + tb);
    w.st0 = reinterpret_cast<int *>(base + 2 * tb);
    const int nf = A.F.n_fleets;
    for (int64_t b = int64_t(blockIdx.x) * kPer; b < nf; b += int64_t(gridDim.x) * kPer) {
        const int64_t f = b + seg;
        if (f < nf) sweep_fleet<true, false, Seg<kSegLanes>>(A, A.F, A.out, int(f), w, sg);
    }
}

// halda_sweep_kslot_kernel: the k-sweep of fleets of at most kSegLanes devices (C2) with the k's
// spread over waves. A workgroup holds four fleets (one per 16-lane segment, as the segment kernel)
// and one wave per open k-slot (the k's some fleet of the batch can take: L / k >= min_devices,
// L / k < 1e6, ascending); wave q solves k-slot q of its four fleets -- the k = 1 register greedy,
// the forced W = M split, or the k > 1 tables + threshold scan in its own LDS slice -- and leaves its
// objective, status and (w, n) in the workgroup's pick area. After one barrier, wave 0 picks each
// fleet's best k by the reference's rule (ascending k, strict "<" on obj_value,
// halda_p_solver.py:407) and writes best_k / obj_value / w / n; the k's no slot takes (settled for
// every fleet: M > W or W >= 1e6) are written there too. Same per-(fleet, k) arithmetic as
// sweep_fleet on Seg<16> (the same records, reductions and tie rules: the same bits), but the
// segment kernel's one wave per four fleets becomes one wave per (four fleets, k): four to sixteen
// times the waves to hide the reductions' and LDS round trips' latency. What the slot waves cannot
// take (greedy fallbacks, tables beyond the slice, non-convex leaves) flags the fleet for the gated
// table launch, which redoes it whole.
constexpr int kMaxSlots = 16;
constexpr int kSlotFlagged = 1000;  // SlotPick.st: the fleet goes to the table launch

struct SlotPick {  // one (segment, k-slot) result in the workgroup's pick area (written after the last use of the
    double obj;    // tables, over them); the slot's (w, n) stay in its wave's registers, and the winning wave
    int st;        // writes them (kslot_pick). st: HALDA_STATUS_* or kSlotFlagged
    int pad;
};

// LDS bytes of one segment's slice of a k-slot (none for a slot without tables: the k = 1 greedy and the
// forced W = M split run in registers).
__host__ __device__ inline int64_t kslot_slice_bytes(int mmax, int tab) {
    return tab > 0 ? seg_slice_bytes(mmax, tab) : 0;
}

struct SlotArgs {
    int n_slot;
    int pick_off;              // LDS byte offset of the pick area (SlotPick [4][n_slot]; over the tables, dead by then)
    int j[kMaxSlots];          // k index of slot q (ascending)
    int tab[kMaxSlots];        // doubles of G (and of H) per segment: max_devices * odd_stride(R + 1), 0: no tables
    int r1[kMaxSlots];         // largest R + 1 of slot q over the batch
    int off[kMaxSlots];        // LDS byte offset of slot q's four segment slices
    int helper;                // slot whose threshold scan is split over n_parts waves (-1: none)
    int n_parts;               // 2 (split) or 0
    int part_wave[kMaxSplitParts - 1];  // the wave that takes part 2 first: a light slot's, or n_slot
    int split_off;             // LDS byte offset of the split areas (SplitArea [4])
    int rec_off;               // LDS byte offset of the workgroup's device records (KslotRecs; over the tables,
                               // which are written only after every wave has read its records)
    int check_wave;            // the wave that checks the split slot's leaves after its own slot (-1: none)
    int opt;                   // 1: an optimistic part 1 where its rows allow (0: the sequential order, a test path)
    int crit_w4;               // table share of the critical slot's wave, in quarters of the others'
    int cut8;                  // the split scan's cut: rank cut8 / 8 of the way up (ScanSplit::cut8)
};
static_assert(kSegLanes == 16, "SplitArea holds 16 lanes per segment");

// Waves of a k-slot workgroup: one per slot, plus an extra helper wave when no other slot can host one.
__host__ __device__ inline int kslot_waves(const SlotArgs &SA) {
    return SA.n_slot + (SA.helper >= 0 && SA.part_wave[0] == SA.n_slot ? 1 : 0);
}

// Part (2 or 3) of the split scan this wave takes first, 0: none.
__device__ inline int kslot_part_of(const SlotArgs &SA, int q) {
    if (SA.helper < 0) return 0;
    for (int h = 0; h < SA.n_parts - 1; ++h)
        if (SA.part_wave[h] == q) return h + 2;
    return 0;
}

// One (fleet, k_j) on a 16-lane segment; the result goes to *pk (segment lane 0 writes obj / st, lane i
// its w / n candidate).
// One fleet of a k-slot workgroup, in registers: its extent, this lane's device record and the
// objective constants (every wave of the workgroup builds the same, from one round of field loads).
struct KslotFleet {
    int64_t d0;
    int M;
    FieldRec me;
    double tsum, xsum, kappa;
    bool anybad;
};

// The workgroup's device records in LDS: wave 0 forms them (kslot_records) and every other wave of
// the workgroup reads them, instead of each wave loading the fields and forming the same records again
// (they are the same four fleets for every slot wave).
struct KslotRecs {
    double alpha[64], b[64], p_bp[64], p_b[64], cst[64];
    int Kset[64], Kvram[64], cg[64];  // cg: cls | gpu << 4
    double tsum[64 / kSegLanes], kappa[64 / kSegLanes];
    int anybad[64 / kSegLanes];
};

__device__ inline void kslot_put_records(KslotRecs *R, const KslotFleet &fd, int lane, int seg) {
    R->alpha[lane] = fd.me.alpha; R->b[lane] = fd.me.b; R->p_bp[lane] = fd.me.p_bp; R->p_b[lane] = fd.me.p_b;
    R->cst[lane] = fd.me.cst;
    R->Kset[lane] = fd.me.Kset; R->Kvram[lane] = fd.me.Kvram; R->cg[lane] = fd.me.cls | (fd.me.gpu << 4);
    if (lane % kSegLanes == 0) {
        R->tsum[seg] = fd.tsum;
        R->kappa[seg] = fd.kappa;
        R->anybad[seg] = fd.anybad ? 1 : 0;
    }
}

__device__ inline KslotFleet kslot_get_records(const SweepArgs &A, const halda_fleets &F, const KslotRecs *R, int f,
                                               int lane, int seg) {
    KslotFleet fd;
    fd.d0 = A.uM > 0 ? int64_t(f) * A.uM + F.dev_off[0] : F.dev_off[f];
    fd.M = A.uM > 0 ? A.uM : int(F.dev_off[f + 1] - fd.d0);
    fd.me.alpha = R->alpha[lane]; fd.me.b = R->b[lane]; fd.me.p_bp = R->p_bp[lane]; fd.me.p_b = R->p_b[lane];
    fd.me.cst = R->cst[lane];
    fd.me.Kset = R->Kset[lane]; fd.me.Kvram = R->Kvram[lane];
    const int cg = R->cg[lane];
    fd.me.cls = cg & 15;
    fd.me.gpu = cg >> 4;
    fd.me.W = 0;
    fd.tsum = R->tsum[seg];
    fd.xsum = 0.0;  // fleet_offsets_regs carries every per-device constant in tsum
    fd.kappa = R->kappa[seg];
    fd.anybad = R->anybad[seg] != 0;
    return fd;
}

__device__ inline KslotFleet kslot_records(const SweepArgs &A, const halda_fleets &F, int f, const Seg<kSegLanes> &sg) {
    KslotFleet fd;
    const int lane = sg.sl;
    fd.d0 = A.uM > 0 ? int64_t(f) * A.uM + F.dev_off[0] : F.dev_off[f];
    fd.M = A.uM > 0 ? A.uM : int(F.dev_off[f + 1] - fd.d0);
    const DevFields mf = load_fields(F, fd.d0 + (lane < fd.M ? lane : 0));
    int bad = 0;
    fd.me = field_rec(A.Mo, mf, bad);
    bad = lane < fd.M ? bad : 0;
    fleet_offsets_regs(A.Mo, mf, fd.M, sg, fd.tsum, fd.xsum, fd.kappa);
    fd.anybad = sg.any(bad != 0);
    return fd;
}

// The (fleet, k_j) instance solves through the tables + threshold scan (not the register greedy /
// forced split, not flagged): the same conditions sweep_kslot's branches test.
__device__ inline bool kslot_uses_tables(const KslotFleet &fd, int k, int W, int r1cap, int tabcap, int mmax) {
    if (!(W < 1000000) || fd.M > W || fd.anybad || k == 1 || W == fd.M || fd.M < 2) return false;
    const int R1 = W - fd.M + 1;
    return fd.M <= mmax && R1 <= r1cap && int64_t(fd.M) * odd_stride(R1) <= tabcap;
}

// Slot p's LDS slice of this segment.
__device__ inline WaveCtx kslot_ctx(const SweepArgs &A, const SlotArgs &SA, int p, unsigned char *smem, int seg) {
    const int tab = SA.tab[p];
    const int64_t tb = align16(int64_t(tab) * 8);
    unsigned char *base = smem + SA.off[p] + int64_t(seg) * kslot_slice_bytes(A.mmax, tab);
    WaveCtx w = {};
    w.G = reinterpret_cast<double *>(base);
    w.H = reinterpret_cast<double *>(base + tb);
    w.st0 = reinterpret_cast<int *>(base + 2 * tb);
    return w;
}

// Phase B of the k-slot workgroup: every wave builds an equal share of ALL the slots' k > 1 tables
// (the (slot, entry) pairs in slot order, cut into one contiguous stretch per wave; lane = device; each
// stretch starts with a full split search, the same least minimisers as one chain, so the same
// tables), instead of each k > 1 wave building its own while the W = M / k = 1 waves idle at the
// barrier: the longest wave's dependent chain loses its table pass.
__device__ void kslot_tables(const SweepArgs &A, const SlotArgs &SA, int q, int crit, const KslotFleet &fd,
                             const Seg<kSegLanes> &sg, unsigned char *smem, int seg) {
    const int lane = sg.sl;
    int total = 0;
    for (int p = 0; p < SA.n_slot; ++p) total += SA.tab[p] > 0 ? SA.r1[p] : 0;
    const int nw = kslot_waves(SA);
    // wave weights in quarters: 4 each, crit_w4 for the critical slot's wave (issue priority: it
    // builds faster and would otherwise wait at the barrier)
    const int cw = crit >= 0 ? SA.crit_w4 : 4;
    const int64_t wt = 4 * int64_t(nw) + cw - 4;
    auto before = [&](int r) { return 4 * int64_t(r) + (crit >= 0 && crit < r ? cw - 4 : 0); };
    const int lo = int(total * before(q) / wt), hi = int(total * before(q + 1) / wt);
    int base = 0;
    for (int p = 0; p < SA.n_slot; ++p) {
        if (SA.tab[p] <= 0) continue;
        const int b0 = base;
        base += SA.r1[p];
        const int a = max(lo, b0) - b0, b = min(hi, base) - b0;
        if (a >= b) continue;
        const int k = A.ks[SA.j[p]], W = A.Ws[SA.j[p]];
        if (!kslot_uses_tables(fd, k, W, SA.r1[p], SA.tab[p], A.mmax)) continue;
        Inst I = {};
        I.M = fd.M;
        I.W = W;
        I.Wd = double(W);
        I.kc = double(k - 1);
        I.iC = 7 * fd.M;
        I.R1 = W - fd.M + 1;
        I.RS = odd_stride(I.R1);
        const WaveCtx w = kslot_ctx(A, SA, p, smem, seg);
        FieldRec rec = fd.me;
        rec.W = W;
        if (lane < fd.M) {
            int n = 0;
            bool have = false;
            for (int e = a; e < min(b, I.R1); ++e) table_entry(rec, w, I, lane, e, n, have);
        }
    }
}

__device__ void sweep_kslot(const SweepArgs &A, const SweepBatch &B, const KslotFleet &fd, int f, int j, int r1cap,
                            int tabcap, const WaveCtx &w, const Seg<kSegLanes> &sg, SlotPick &pk,
                            unsigned long long *t_rec, const ScanSplit sp, int &wl, int &nl) {
    using SG = Seg<kSegLanes>;
    constexpr int S = SG::S;
    const int lane = sg.sl;
    const int M = fd.M;
    FieldRec me = fd.me;
    const double tsum = fd.tsum, xsum = fd.xsum, kappa = fd.kappa;
    const bool anybad = fd.anybad;
#ifndef HALDA_STAMPS
    (void)t_rec;
#endif
    const int k = A.ks[j], W = A.Ws[j];
    const int64_t inst = int64_t(f) * A.n_k + j;
    const double kc = double(k - 1);
    int st;
    double obj = kInf;
    wl = 0;  // this lane's (w, n) in the solution
    nl = 0;
    if (!(W < 1000000)) st = HALDA_STATUS_UNSUPPORTED;
    else if (M > W) st = HALDA_STATUS_INFEASIBLE;  // sum lb(w) = M > W (HiGHS presolve)
    else if (anybad) st = HALDA_STATUS_UNSUPPORTED;
    else {
        me.W = W;
        if (k == 1 || W == M) {
            // the register greedy; W = M (R = 0): every w_i = 1 is forced
            int e = 0, rounds = 0, nE = 0;
            double gE = 0.0;
            const int rc = k1_alloc(me, M, W - M, sg, e, rounds, gE, nE);
            if (rc == K1_INFEASIBLE) {
                st = HALDA_STATUS_INFEASIBLE;
            } else if (rc == K1_OK) {
                double g = 0.0, H = 0.0, z = 0.0;
                int n = 0, sl[4] = {0, 0, 0, 0};
                wl = 1 + e;
                const bool need_h = kc != 0.0 || (A.outs & kOutX);
                if (lane < M) {
                    g = gE;
                    n = nE;
                    rec_slacks(me, wl, n, sl);
                    if (need_h) {
                        double P, Q;
                        dev_cycle(me, wl, n, sl, P, Q);
                        z = Q > P ? 0.5 * (Q - P) : 0.0;
                        H = Q >= P ? 0.5 * (P + Q) : P;
                    }
                }
                const double hmax = need_h ? fmax(0.0, sg.max_f64(lane < M ? H : 0.0)) : 0.0;
                obj = sg.sum_f64(lane < M ? g : 0.0) + kc * hmax;
                obj = obj + tsum;
                obj = obj + xsum;
                obj = obj + kappa;
                st = HALDA_STATUS_OPTIMAL;
                nl = n;
                if (lane < M) put_xc(A, B.out, inst, M, lane, wl, n, sl, z, me);
                if (lane == 0 && (A.outs & kOutXC)) {
                    const int64_t at = xc_at(A, inst);
                    if (at >= 0 && (A.outs & kOutX)) B.out.x[at + 7 * M] = hmax;
                    if (at >= 0 && (A.outs & kOutC)) B.out.c[at + 7 * M] = kc;
                }
            } else {
                st = kSlotFlagged;  // a greedy fallback: the 64-lane table launch
            }
        } else if (M < 2) {
            st = kSlotFlagged;
        } else {
            Inst I = {};
            I.inst = int(inst);
            I.M = M;
            I.W = W;
            I.Wd = double(W);
            I.kc = kc;
            I.iC = 7 * M;
            I.R1 = W - M + 1;
            I.RS = odd_stride(I.R1);
            if (M > A.mmax || I.R1 > r1cap || int64_t(M) * I.RS > tabcap) {
                st = kSlotFlagged;  // beyond the slot's slice
            } else {
                // the tables were built by the whole workgroup (kslot_tables, before the barrier)
                int64_t nodes = 0;
                const int feas = dp_pass_lanes(w, I, sg, nodes, t_rec + 4, sp);
#ifdef HALDA_STAMPS
                t_rec[2] = __builtin_amdgcn_s_memtime();
                t_rec[3] = (unsigned long long)nodes;
#endif
                if (feas < 0) {
                    st = kSlotFlagged;  // a leaf the incremental scan does not take
                } else if (!feas) {
                    st = HALDA_STATUS_INFEASIBLE;
                } else {
                    double g = 0.0, P = 0.0, Q = 0.0, hmax = 0.0;
                    int n = 0, sl[4] = {0, 0, 0, 0};
                    if (lane < M) {
                        wl = 1 + w.st0[lane];
                        split_full(me, wl, g, n, sl);
                        dev_cycle(me, wl, n, sl, P, Q);
                        hmax = Q >= P ? 0.5 * (P + Q) : P;
                        put_xc(A, B.out, inst, M, lane, wl, n, sl, Q > P ? 0.5 * (Q - P) : 0.0, me);
                    }
                    hmax = sg.max_f64(fmax(0.0, hmax));
                    obj = sg.sum_f64(0.0 + g) + kc * hmax;  // the segment kernel's sum (0.0 + g per lane)
                    obj = obj + tsum;
                    obj = obj + xsum;
                    obj = obj + kappa;
                    st = HALDA_STATUS_OPTIMAL;
                    nl = n;
                    if (lane == 0 && (A.outs & kOutXC)) {
                        const int64_t at = xc_at(A, inst);
                        if (at >= 0 && (A.outs & kOutX)) B.out.x[at + 7 * M] = hmax;
                        if (at >= 0 && (A.outs & kOutC)) B.out.c[at + 7 * M] = kc;
                    }
                }
            }
        }
    }
    if (st == kSlotFlagged) {
        flag_fleet(A, B.fflag, f, lane);
    } else {
        if (lane == 0) {
            if (A.outs & kOutObk) B.out.obj_by_k[inst] = st == HALDA_STATUS_OPTIMAL ? obj : kInf;
            if (A.outs & kOutSt) B.out.status[inst] = st;
        }
        if ((A.outs & kOutXZ) && st != HALDA_STATUS_OPTIMAL && (A.outs & kOutXC)) {  // x / c of a non-optimal instance
            const int64_t at = xc_at(A, inst);
            if (at >= 0)
                for (int cc = lane; cc < 7 * M + 1; cc += S) {
                    if (A.outs & kOutX) B.out.x[at + cc] = 0.0;
                    if (A.outs & kOutC) B.out.c[at + cc] = 0.0;
                }
        }
    }
    pk.obj = st == HALDA_STATUS_OPTIMAL ? obj : kInf;  // (lane 0's are the segment's)
    pk.st = st;
}

// The pick of one fleet (segment lanes), run by every slot wave q after the last barrier: best k over the
// slots in ascending k with strict "<"; the winning slot's wave writes its (w, n) from its registers (wl,
// nl), wave 0 the settled k's of no slot, best_k / obj_value, the fleet's flag byte and, when no k is
// feasible, zero (w, n).
__device__ void kslot_pick(const SweepArgs &A, const SweepBatch &B, const SlotArgs &SA, int f, const SlotPick *pk,
                           const Seg<kSegLanes> &sg, int q, int wl, int nl) {
    constexpr int S = kSegLanes;
    const int lane = sg.sl;
    const int64_t d0 = A.uM > 0 ? int64_t(f) * A.uM + B.F.dev_off[0] : B.F.dev_off[f];
    const int M = A.uM > 0 ? A.uM : int(B.F.dev_off[f + 1] - d0);
    bool flagged = false;
    double best = kInf;
    int bq = -1;
    for (int q = 0; q < SA.n_slot; ++q) {
        const int st = pk[q].st;
        flagged = flagged || st == kSlotFlagged;
        if (st == HALDA_STATUS_OPTIMAL && pk[q].obj < best) {
            best = pk[q].obj;
            bq = q;
        }
    }
    if (flagged) return;  // the table launch redoes this fleet (fflag / hb_flag set by the slot wave)
    if (q == bq && lane < M) {
        B.out.w[d0 + lane] = wl;
        B.out.n[d0 + lane] = nl;
    }
    if (q != 0) return;
    // k's of no slot: settled for every fleet of the batch (W >= 1e6 unsupported, else M > W)
    for (int jj = lane; jj < A.n_k; jj += S) {
        bool slot = false;
        for (int q = 0; q < SA.n_slot; ++q) slot = slot || SA.j[q] == jj;
        if (slot) continue;
        const int64_t inst = int64_t(f) * A.n_k + jj;
        const int st = !(A.Ws[jj] < 1000000) ? HALDA_STATUS_UNSUPPORTED : HALDA_STATUS_INFEASIBLE;
        if (A.outs & kOutObk) B.out.obj_by_k[inst] = kInf;
        if (A.outs & kOutSt) B.out.status[inst] = st;
        if ((A.outs & kOutXZ) && (A.outs & kOutXC)) {
            const int64_t at = xc_at(A, inst);
            if (at >= 0)
                for (int cc = 0; cc < 7 * M + 1; ++cc) {
                    if (A.outs & kOutX) B.out.x[at + cc] = 0.0;
                    if (A.outs & kOutC) B.out.c[at + cc] = 0.0;
                }
        }
    }
    if (lane == 0) {
        B.out.best_k[f] = bq >= 0 ? A.ks[SA.j[bq]] : 0;
        B.out.obj_value[f] = best;
        B.fflag[f] = 0;
    }
    if (bq < 0 && lane < M) {
        B.out.w[d0 + lane] = 0;
        B.out.n[d0 + lane] = 0;
    }
}

// The leaf checks of the split slot's rows for an optimistic part 1 (dp_pass_lanes takes rows finite at
// both ends as [0, R1 - 1] without checking them and awaits this verdict before it returns): made by
// SA.check_wave after its own slot, the wave whose slot ends first, while part 1 scans.
__device__ void kslot_check(const SweepArgs &A, const SlotArgs &SA, const KslotFleet &fd, SplitArea *ar,
                            const Seg<kSegLanes> &sg, unsigned char *smem, int seg, bool live) {
    const int p = SA.helper, lane = sg.sl;
    const int j = SA.j[p], k = A.ks[j], W = A.Ws[j];
    if (!SA.opt || !live || !kslot_uses_tables(fd, k, W, SA.r1[p], SA.tab[p], A.mmax)) return;
    const int M = fd.M, R1 = W - M + 1, RS = odd_stride(R1);
    const bool act = lane < M;
    const WaveCtx w = kslot_ctx(A, SA, p, smem, seg);
    const double *G = w.G + int64_t(act ? lane : 0) * RS, *H = w.H + int64_t(act ? lane : 0) * RS;
    if (!leaf_ends_finite(G, R1, act, sg)) return;  // part 1 checks these itself
    int lo = R1, hi = -1, cnt = 0;
    bool ok = true, mono = true;
    leaf_scan(G, H, R1, act, lo, hi, cnt, ok, mono);
    const int v = sg.any(act && (!ok || !mono)) ? 2 : 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(&ar->verdict, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A helper wave of a k-slot workgroup, after its own slot: its part (T range) of the split slot's
// threshold scan for its segment's fleet, from what part 1 published after its leaf scan and phase-0
// greedy (part 1 publishes on every path: "skip" when it does not scan), into the split area; then
// the flag, on every path (part 1 waits for it only when it scanned). The wait is a wave-uniform
// polling loop in which every segment whose publication is in runs its part at once: a segment must
// never wait behind another one of the same wave (part 1 may publish that one only after its own
// scan, which waits for this segment's flag).
__device__ void kslot_helper(const SweepArgs &A, const SlotArgs &SA, const KslotFleet &fd, SplitArea *ar, int part,
                             const Seg<kSegLanes> &sg, unsigned char *smem, int seg, bool live) {
    const int p = SA.helper, h = part - 2, lane = sg.sl;
    const int j = SA.j[p], k = A.ks[j], W = A.Ws[j];
    // part 1 reaches its leaf scan (else it publishes nothing this wave needs: post at once)
    bool pending = live && kslot_uses_tables(fd, k, W, SA.r1[p], SA.tab[p], A.mmax);
    if (live && lane == 0) ar->alt_best[h] = kInf;
    // an optimistic part 1 (rows finite at both ends: dp_pass_lanes) leaves phase 0 to this wave: the
    // unconstrained allocation into the split slot's st0, then the publication part 1's scan awaits
    if (h == 0 && pending) {
        const int M = fd.M, R1 = W - M + 1, RS = odd_stride(R1);
        const bool act = lane < M;
        const WaveCtx w = kslot_ctx(A, SA, p, smem, seg);
        const double *G = w.G + int64_t(act ? lane : 0) * RS, *H = w.H + int64_t(act ? lane : 0) * RS;
        if (SA.opt && leaf_ends_finite(G, R1, act, sg)) {
            const int hi = act ? R1 - 1 : -1;
            int e = 0;
            phase0_greedy(w.G, RS, R1 - 1, sg, act, hi, e);
            const double s_inf = sg.sum_f64(act ? G[e] : 0.0);
            const double hmax = sg.max_f64(act ? fmax(0.0, H[e]) : 0.0);
            if (act) w.st0[lane] = e;
            split_publish(ar, lane, act, act ? 0 : R1, hi, s_inf, double(k - 1) * hmax + s_inf, 0,
                          sg.sum_i(act ? R1 - 1 : 0));
        }
    }
    while (__ballot(pending)) {
        const int pb = pending ? __hip_atomic_load(&ar->pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
        if (pending && pb != 0) {  // segment-uniform
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (pb == 1) {
                Inst I = {};
                I.M = fd.M;
                I.W = W;
                I.Wd = double(W);
                I.kc = double(k - 1);
                I.iC = 7 * fd.M;
                I.R1 = W - fd.M + 1;
                I.RS = odd_stride(I.R1);
                const bool act = lane < fd.M;
                LeafInfo li = {};
                li.convex = true;  // part 1 checked every leaf before it published
                li.mono = true;
                li.empty = false;
                li.lo_sum = ar->lo_sum;
                li.cap = ar->capsum;
                li.my_lo = act ? ar->lo[lane] : 0;
                li.my_hi = act ? ar->hi[lane] : -1;
                WaveCtx w = kslot_ctx(A, SA, p, smem, seg);
                w.st0 = ar->alt_e[h];  // this part's result, not the slot's st0
                int64_t nodes = 0;
                ScanSplit sp{part, SA.n_parts, ar};
                sp.cut8 = SA.cut8;
                (void)kc_scan_incremental(w, I, sg, ar->s_inf, ar->best0, nodes, li, sp);
            }
            pending = false;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&ar->flag[h], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (pending) {
            __builtin_amdgcn_s_sleep(2);
        }
    }
    if (live && !kslot_uses_tables(fd, k, W, SA.r1[p], SA.tab[p], A.mmax)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __hip_atomic_store(&ar->flag[h], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// The slot with the largest k > 1 tables (C2: k = 2): the workgroup's critical path, its threshold scan
// the last thing running; -1 when no slot has tables.
__device__ inline int kslot_crit(const SlotArgs &SA) {
    int crit = -1, r1 = 0;
    for (int p = 0; p < SA.n_slot; ++p)
        if (SA.tab[p] > 0 && SA.r1[p] > r1) {
            r1 = SA.r1[p];
            crit = p;
        }
    return crit;
}

// One k-slot workgroup's four fleets (group g: fleets 4 g .. 4 g + 3 of batch B), every slot wave: the
// records (wave 0, shared through LDS), the tables, each slot's solve and the split scan's parts, the
// pick. Three workgroup barriers on every wave's path.
__device__ void kslot_group(const SweepArgs &A, const SlotArgs &SA, const SweepBatch &B, int64_t g,
                            unsigned char *smem, int crit) {
    constexpr int kPer = 64 / kSegLanes;
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // this wave's k-slot
    const Seg<kSegLanes> sg(lane);
    const int seg = lane / kSegLanes;
    const int nf = B.F.n_fleets;
    const int64_t f = g * kPer + seg;
    SlotPick *pick = reinterpret_cast<SlotPick *>(smem + SA.pick_off);
    // the critical slot's wave gets the SIMD's issue priority over the other slots' waves (of other
    // workgroups) it shares the SIMD with (its helpers once their own slot is done)
    if (q == crit) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(0);  // (a helper's raised priority ends with its group)
    SplitArea *split = reinterpret_cast<SplitArea *>(smem + SA.split_off) + seg;
    HALDA_KSTAMPW(0, __builtin_amdgcn_s_memtime());
    // slot 5: the constant-rate clock at start (low 40 bits), the wave's HW_ID[15:0] (SIMD, CU, SE) and
    // XCC_ID[3:0] above
    HALDA_KSTAMPW(5, (__builtin_amdgcn_s_memrealtime() & ((1ull << 40) - 1)) |
                         (uint64_t(__builtin_amdgcn_s_getreg((15 << 11) | 4)) << 40) |
                         (uint64_t(__builtin_amdgcn_s_getreg((3 << 11) | 20)) << 56));
    {
        // the four fleets' device records: formed by wave 0 alone, shared through LDS
        KslotRecs *recs = reinterpret_cast<KslotRecs *>(smem + SA.rec_off);
        KslotFleet fd = {};
        if (q == 0) {
            if (f < nf) {
                fd = kslot_records(A, B.F, int(f), sg);
                kslot_put_records(recs, fd, lane, seg);
            }
        }
        __syncthreads();  // the records are in LDS
        if (q != 0 && f < nf) fd = kslot_get_records(A, B.F, recs, int(f), lane, seg);
        __syncthreads();  // every wave has its records: the tables below may overwrite them
        HALDA_KSTAMPW(1, __builtin_amdgcn_s_memtime());
        if (f < nf) kslot_tables(A, SA, q, crit, fd, sg, smem, seg);
        const int my_part = kslot_part_of(SA, q);
        if (my_part && sg.sl == 0) split->flag[my_part - 2] = 0;  // posted after the barrier
        if (q == SA.helper && sg.sl == 0) {
            split->pub = 0;
            split->verdict = 0;
        }
        HALDA_KSTAMPW(6, __builtin_amdgcn_s_memtime());
        __syncthreads();  // every slot's tables are complete
        HALDA_KSTAMPW(11, __builtin_amdgcn_s_memtime());
        if (q == SA.n_slot) {  // an extra helper wave: no slot of its own
            __builtin_amdgcn_s_setprio(3);
            if (q == SA.check_wave) kslot_check(A, SA, fd, split, sg, smem, seg, f < nf);
            kslot_helper(A, SA, fd, split, my_part, sg, smem, seg, f < nf);
            __syncthreads();  // the pick barriers below
            __syncthreads();
            return;
        }
        const WaveCtx w = kslot_ctx(A, SA, q, smem, seg);
#ifdef HALDA_STAMPS_DUMP  // (-DHALDA_STAMPS -DHALDA_STAMPS_DUMP: tools/kslot_tables.py)
        if (f < kDumpFleets && A.ks[SA.j[q]] == 2 && SA.tab[q] > 0 && lane % kSegLanes < fd.M) {
            const int R1 = A.Ws[SA.j[q]] - fd.M + 1, RS = odd_stride(R1), i = lane % kSegLanes;
            for (int e = 0; e < kDumpE; ++e) {
                const int64_t o = ((int64_t(f) * kDumpDev + i) * kDumpE + e) * 2;
                g_halda_dump[o] = e < R1 ? w.G[i * RS + e] : kInf;
                g_halda_dump[o + 1] = e < R1 ? w.H[i * RS + e] : kInf;
            }
        }
#endif
        unsigned long long t_rec[6] = {0, 0, 0, 0, 0, 0};
        int wl = 0, nl = 0;
        SlotPick mine = {kInf, HALDA_STATUS_INFEASIBLE, 0};
#ifdef HALDA_STAMPS
        ScanSplit sp{q == SA.helper ? 1 : 0, SA.n_parts, split, false, SA.opt != 0,
                     int64_t(blockIdx.x) * SA.n_slot + q < kStampInst
                         ? g_halda_scanprof + (int64_t(blockIdx.x) * SA.n_slot + q) * kScanProf
                         : nullptr};
#else
        ScanSplit sp{q == SA.helper ? 1 : 0, SA.n_parts, split, false, SA.opt != 0};
#endif
        sp.cut8 = SA.cut8;
        if (f < nf)
            sweep_kslot(A, B, fd, int(f), SA.j[q], SA.r1[q], SA.tab[q], w, sg, mine, t_rec, sp, wl, nl);
        if (q == SA.helper && f < nf && sg.sl == 0 && split->pub == 0) split->pub = 2;  // did not scan: helpers skip
        if (q == SA.check_wave) kslot_check(A, SA, fd, split, sg, smem, seg, f < nf);
        if (my_part) {  // after its own slot, at the split slot's priority
            __builtin_amdgcn_s_setprio(3);
            kslot_helper(A, SA, fd, split, my_part, sg, smem, seg, f < nf);
        }
        HALDA_KSTAMPW(7, t_rec[2]);
        HALDA_KSTAMPW(8, t_rec[3]);
        HALDA_KSTAMPW(9, t_rec[4]);
        HALDA_KSTAMPW(10, t_rec[5]);
        HALDA_KSTAMPW(2, __builtin_amdgcn_s_memtime());
        __syncthreads();  // every table read is done: the pick area over them is free
        if (f < nf && sg.sl == 0) pick[seg * SA.n_slot + q] = mine;
        __syncthreads();
        HALDA_KSTAMPW(3, __builtin_amdgcn_s_memtime());
        if (f < nf) kslot_pick(A, B, SA, int(f), pick + seg * SA.n_slot, sg, q, wl, nl);
        HALDA_KSTAMPW(4, __builtin_amdgcn_s_memtime());
    }
}

__global__ __launch_bounds__(64 * kMaxSlots) void halda_sweep_kslot_kernel(SweepArgs A, SlotArgs SA) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    kslot_group(A, SA, batch_of(A), int64_t(blockIdx.x), smem, kslot_crit(SA));
}

// halda_sweep_kslot_steps_kernel: `steps` batches of k-slot sweeps (C2 shapes) in one launch, the group
// launch's k-slot form: one workgroup per item (batch t = blockIdx.y, group of four fleets), so the
// hardware dispatcher hands the next item to whichever CU frees its resources first -- the launch is
// paced by the mean group, not by the slowest of the 1,024 resident at once -- with the per-batch
// kernel's registers (no item loop). Item (t, gg) solves group g = (gg + t * kKslotRot) mod n_groups (a
// bijection per batch), which spreads a slow group's batches over the launch. Fleets a slot flags go to
// the per-batch flag array; halda_sweep_tables_steps_kernel redoes them after the launch.
constexpr int kKslotRot = 389;

__global__ __launch_bounds__(64 * kMaxSlots) void halda_sweep_kslot_steps_kernel(SweepArgs A, SlotArgs SA, StepsArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nf = A.F.n_fleets;
    const int ng = int(gridDim.x);
    const int t = int(blockIdx.y), gg = int(blockIdx.x);
    // 32-bit: gg < ng, t < 65,536, first < n_desc
    const int g = int((unsigned(gg) + unsigned(t) * unsigned(kKslotRot)) % unsigned(ng));
    const int b = int((unsigned(G.first) + unsigned(t)) % unsigned(G.n_desc));
    kslot_group(A, SA, SweepBatch{steps_fleets(steps_desc(G, b)), steps_out(steps_desc(G, b)), G.fflag + int64_t(b) * nf},
                g, smem, kslot_crit(SA));
}

// The gated table launch behind a k-slot steps launch: blockIdx.y = the group entry (first + y) mod
// n_desc, the fleets its items flagged (gated on the launch's hand-back flag).
__global__ __launch_bounds__(64, HALDA_SOLVE_WAVES_PER_SIMD) void halda_sweep_tables_steps_kernel(SweepArgs A,
                                                                                                StepsArgs G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = int((unsigned(G.first) + blockIdx.y) % unsigned(G.n_desc));
    const halda_fleets F = steps_fleets(steps_desc(G, b));
    const FleetOut O = steps_out(steps_desc(G, b));
    sweep_body<true, false>(A, SweepBatch{F, O, G.fflag + int64_t(b) * A.F.n_fleets}, smem);
}

// halda_pick_kernel: one wave per fleet. obj_value per k = c.x + sum t_comm +
// sum xi + kappa (halda_p_solver.py:356-357), best k by ascending k with strict
// "<" (halda_p_solver.py:407), w / n of the winner (int(round(x)), :350-351).
__global__ __launch_bounds__(64) void halda_pick_kernel(halda_batch B, halda_result R, halda_fleets F, int n_k,
                                                        const double *offs, halda_fleet_result out, int64_t xstride) {
    const int lane = threadIdx.x;
    const int f = blockIdx.x;
    if (f >= F.n_fleets) return;
    int best_j = -1;
    double best = kInf;
    for (int j = 0; j < n_k; ++j) {
        const int64_t inst = int64_t(f) * n_k + j;
        const int st = R.status[inst];
        double obj = kInf;
        if (st == HALDA_STATUS_OPTIMAL) {
            const int64_t co = B.col_off[inst];
            const int N = B.n_cols[inst];
            double part = 0.0;
            for (int c = lane; c < N; c += 64) part += B.c[co + c] * R.x[co + c];
            obj = wave_sum_f64(part);
            obj = obj + offs[3 * f + 0];
            obj = obj + offs[3 * f + 1];
            obj = obj + offs[3 * f + 2];
            if (obj < best) {
                best = obj;
                best_j = j;
            }
        }
        if (lane == 0) {
            if (out.obj_by_k) out.obj_by_k[inst] = obj;
            if (out.status) out.status[inst] = st;
        }
        const int64_t at = out.x_off ? out.x_off[inst] : inst * xstride;
        if ((out.x || out.c) && at >= 0) {
            const int64_t co = B.col_off[inst];
            const int N = B.n_cols[inst];
            for (int cc = lane; cc < N; cc += 64) {
                if (out.x) out.x[at + cc] = st == HALDA_STATUS_OPTIMAL ? R.x[co + cc] : 0.0;
                if (out.c) out.c[at + cc] = st == HALDA_STATUS_OPTIMAL ? B.c[co + cc] : 0.0;
            }
        }
    }
    const int64_t d0 = F.dev_off[f];
    const int M = int(F.dev_off[f + 1] - d0);
    if (lane == 0) {
        out.best_k[f] = best_j >= 0 ? int(B.c[B.col_off[int64_t(f) * n_k + best_j] + 7 * M]) + 1 : 0;
        out.obj_value[f] = best;
    }
    for (int i = lane; i < M; i += 64) {
        int w = 0, n = 0;
        if (best_j >= 0) {
            const int64_t co = B.col_off[int64_t(f) * n_k + best_j];
            w = int(rint(R.x[co + i]));
            n = int(rint(R.x[co + M + i]));
        }
        out.w[d0 + i] = w;
        out.n[d0 + i] = n;
    }
}
