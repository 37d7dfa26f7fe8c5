// libhalda — exact batched solver for fixed-k HALDA MILPs on MI355X (gfx950).
//
// Replaces the per-(fleet, k) call scipy.optimize.milp -> HiGHS made by the
// reference at src/distilp/solver/halda_p_solver.py:340-346 (halda_solve_batch) and
// the whole halda_solve k-sweep of :369-436 (halda_solve_fleets); the C ABI is in
// include/halda.h, the design (and why the solve is exact) in DESIGN.md.
//
// One translation unit in six files:
//   halda_prims.hpp  constants, stamps, LDS slices, wave / segment reductions;
//   halda_solve.hpp  the milp() replacement: records, splits, greedy, DP, CSR decode,
//                    screen / k = 1 / general kernels;
//   halda_sweep.hpp  the k-sweep: GPU lowering, fused sweep kernels, k-slot kernel, pick;
//   halda.hip        host side: contexts, launch sequences, the C ABI, RCCL latency mode;
//   halda_stage.hpp  the host entries' staging layout (no HIP: also built alone by a CPU test);
//   halda_launch.hpp the launch record, the families' path / route knobs, result slices (no HIP either).
// Floating point keeps the reference's operation order (-ffp-contract=off).

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "halda.h"
#include "halda_boxes.h"
#include "halda_launch.hpp"
#include "halda_stage.hpp"

namespace {
// Page-locked host blocks handed out by halda_host_alloc: a call whose every host array lies in one of
// them copies straight between them and device memory (no staging memcpy through the context's buffer).
std::mutex g_host_mu;
std::vector<std::pair<uintptr_t, size_t>> g_host_blocks;

bool in_host_block(const void *p, size_t bytes) {
    if (!p) return true;  // an absent optional array
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lock(g_host_mu);
    for (const auto &b : g_host_blocks)
        if (a >= b.first && a - b.first <= b.second && bytes <= b.second - (a - b.first)) return true;
    return false;
}


#include "halda_prims.hpp"
#include "halda_solve.hpp"
#include "halda_sweep.hpp"

// ------------------------------------------------------------------ host side
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return fail(HALDA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Ctx;
// A prepared plan or group bound to a context: halda_free detaches every live one (c = nullptr), so a
// launch through it after the context is gone fails with HALDA_E_ARG instead of touching freed memory.
struct CtxHandle {
    Ctx *c = nullptr;
};

struct Ctx {
    int device = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evs = nullptr, evk = nullptr;  // start, end, after k = 1, after screen
    bool timed = false;
    bool timing = true;  // record the per-launch HIP events (halda_set_timing)
    int *hb_flag = nullptr;  // launch id of the last launch with a k = 1 hand-back
    int launch_id = 0;
    void *scratch = nullptr;  // host-API staging (device)
    void *pinned = nullptr;   // host-API staging (pinned host), one PCIe copy each way
    void *pinned_dev = nullptr;  // its device address (zero-copy small calls), looked up once
    // the resident single-fleet solver (halda_resident_kernel): its mailbox (fine-grained pinned memory),
    // stream, exit event, the last request number, whether a launch of it may still be running
    ResidentBox *rbox = nullptr;
    void *rbox_dev = nullptr;
    hipStream_t rstream = nullptr;
    hipEvent_t rdone = nullptr;
    uint32_t rseq = 0;
    bool rlive = false;
    bool resident = true;  // HALDA_RESIDENT=0 at halda_init: every small call launches its own kernel
    bool resident_drop = false;  // HALDA_RESIDENT_TEST=drop (fault injection): requests are never posted
    std::vector<void *> retired;  // pinned buffers a resident wave that would not stop may still write
    size_t pinned_bytes = 0;
    size_t scratch_bytes = 0;
    void *work = nullptr;  // cls[n]: screen verdict per instance
    size_t work_bytes = 0;
    void *gtab = nullptr;  // per-wave global-memory slices of the big-table general launch
    size_t gtab_bytes = 0;
    hipEvent_t ev_order = nullptr;  // cross-stream ordering of consecutive launches on this context
    hipEvent_t ev_host = nullptr;   // completion of a small synchronous call (polled, not waited on)
    hipEvent_t evf0 = nullptr, evf1 = nullptr;  // around a halda_solve_fleets sequence (lowering .. pick)
    hipEvent_t evfm = nullptr;                   // fused sweep: between its first and second launch
    lrec::Record fleet_record = lrec::Record::none;  // what the last timed sequence was (halda_last_fleet_ms)
    bool kslot_sweep = true;                     // fused sweep: k-slot launch where it applies (else segment)
    int kslot_split = 2;                         // k-slot launch: the longest scan split over 2 waves (0: unsplit)
    bool kslot_opt = true;                       // ... its part 1 optimistic (leaf checks / phase 0 by other waves)
    int kslot_cut8 = 4;                          // k-slot split scan's cut, eighths (HALDA_KSLOT_CUT8, A/B;
                                                 // 4/8 since five workgroups share a CU: 5/8 before)
    int kslot_pad = 0;                           // HALDA_KSLOT_LDS_PAD (diagnostic): unused LDS bytes per
                                                 // k-slot workgroup, to measure the occupancy's effect
    int kslot_crit_w4 = 8;                       // k-slot table share of the critical slot's wave (quarters; 2x:
                                                 // measured best of 7..12 since part 1 leaves its leaf checks and
                                                 // phase 0 to other waves; 2.5x before)
    bool fleet_timed = false;
    bool fleets_fused = true;      // halda_solve_fleets: the fused sweep (default) or the CSR pipeline
    bool seg_sweep = true;         // fused sweep: lane-segment launch for fleets of <= kSegLanes devices
    bool k1_force_dp = false;      // fused sweep, test path: every register-launch k = 1 solve by k1_dp
    bool x_zero = true;            // fused sweep: x / c of non-optimal instances written as zeros
    bool host_copy = false;        // halda_solve_fleets_host: PCIe copies even for small calls (HALDA_HOST_PATH=copy)
    bool fused_screen = true;      // a settled batch screens inside its k = 1 kernel (HALDA_FUSED_SCREEN=0: screen launch)
    bool fused_last = false;       // the last CSR launch screened in its k = 1 kernel (halda_last_phase_ms)
    int path_gen = 0;              // bumped by halda_set_fleets_path: prepared plans re-plan on their next launch
    void *shard = nullptr;         // rank-local results of halda_solve_fleets_sharded
    size_t shard_bytes = 0;
    void *emu = nullptr;           // the other virtual ranks' results of halda_solve_fleets_sharded_emulated
    size_t emu_bytes = 0;
    // The fused sweep's scratch (per-fleet "needs the table launch" bytes, the hand-back flag) per
    // stream: launches on one stream are ordered by it, so batches enqueued on different streams use
    // different slots and need no cross-stream ordering (they overlap on the device). A slot moving to
    // another stream waits for the launches already enqueued on the stream it leaves.
    struct SweepSlot {
        hipStream_t stream = nullptr;
        bool used = false;
        uint64_t tick = 0;
        uint8_t *fflag = nullptr;
        size_t fflag_bytes = 0;
        uint8_t *cls = nullptr;  // the CSR pipeline's per-instance verdict bytes
        size_t cls_bytes = 0;
        int *hb = nullptr;
        hipEvent_t ev = nullptr;
    };
    static constexpr int kSweepSlots = 8;
    SweepSlot sws[kSweepSlots];
    uint64_t sws_tick = 0;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    void *fleet_scratch = nullptr;  // lowered batch + results of halda_solve_fleets
    size_t fleet_scratch_bytes = 0;
    uint8_t *sub_tab = nullptr;     // halda_solve_subfleets: the expanded table of the expansion route
    size_t sub_tab_bytes = 0;
    uint8_t *sel_buf = nullptr;     // halda_solve_subsets: combo lists, per-(d, fleet) records, per-candidate results
    size_t sel_bytes = 0;
    int64_t scale_chunk = 0;        // halda_set_change_subsets_chunk: a launch's scratch cap (0: the default)
    uint8_t *var_desc = nullptr;    // halda_solve_variants: the fused route's per-variant models (SweepModel)
    size_t var_desc_bytes = 0;
    // Per entry family the path halda_set_<family>_path chose (0: automatic; the admissible codes:
    // lrec::kKnobRules) and the route of the family's last call (0: none yet). Routes -- sub-fleets: 1 fused,
    // 2 expansion; subsets: 1 fused, 2 expansion, 3 mixed; variants: 1 fused, 2 loop; plans: 1 fused, 2 two
    // launches; bounds: 1 fused, 2 general, 3 table launch; boxes: 1 register launch, 3 table launch, 2 loop.
    lrec::Knob knob[lrec::kFamilies];
    halda_batch last_lowered = {};
    halda_result last_solved = {};
    bool have_lowered = false;
    // resident workgroups per CU by (kernel, dynamic LDS), raising the LDS limit once per size
    struct Occ {
        const void *fn;
        int64_t lds;
        int per_cu;
    } occ[8] = {};
    int n_occ = 0;
    // The dynamic-LDS limit is a per-function attribute of the whole process: it only ever rises here
    // (the largest size any plan of any context asked for), so a plan made for a large slice stays
    // launchable after a smaller one was planned for the same kernel.
    // Keyed by (device, kernel) -- contexts on several devices (halda_init_multi) each raise their own --
    // and guarded by a lock: contexts may be driven from different host threads.
    struct LdsAttr {
        int device;
        const void *fn;
        int64_t lds;
    };
    static constexpr int kLdsAttrs = 64;
    static inline std::mutex lds_mu;
    static inline LdsAttr lds_attr[kLdsAttrs] = {};
    static inline int n_lds_attr = 0;
    static hipError_t ensure_lds(const void *fn, int64_t lds) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(lds_mu);
        int i = 0;
        while (i < n_lds_attr && !(lds_attr[i].fn == fn && lds_attr[i].device == dev)) ++i;
        if (i < n_lds_attr && lds_attr[i].lds >= lds) return hipSuccess;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
        if (i == n_lds_attr && n_lds_attr < kLdsAttrs) ++n_lds_attr;
        if (i < kLdsAttrs) lds_attr[i] = LdsAttr{dev, fn, lds};
        return hipSuccess;
    }
    // process-unique (a freed context's address may be reused by the next one): keys the plan cache
    static inline std::atomic<uint64_t> next_uid{1};
    uint64_t uid = next_uid.fetch_add(1);
    std::vector<CtxHandle *> handles;  // live plans / groups made on this context
    void detach(CtxHandle *h) { handles.erase(std::remove(handles.begin(), handles.end(), h), handles.end()); }
    hipError_t occupancy(const void *fn, int64_t lds, int *per_cu) {
        hipError_t e = ensure_lds(fn, lds);
        if (e != hipSuccess) return e;
        for (int i = 0; i < n_occ; ++i)
            if (occ[i].fn == fn && occ[i].lds == lds) {
                if (per_cu) *per_cu = occ[i].per_cu;
                return hipSuccess;
            }
        int p = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&p, fn, 64, size_t(lds));
        if (e != hipSuccess) return e;
        p = std::max(1, p);
        occ[n_occ % 8] = Occ{fn, lds, p};
        n_occ = std::min(n_occ + 1, 8);
        if (per_cu) *per_cu = p;
        return hipSuccess;
    }
};

int64_t slice_bytes_for(int mmax, int r1max, int tab, int tab_kc) {
    return make_slice(mmax, r1max, tab, tab_kc).total;
}

// On-chip budget of one general-kernel slice (LDS per CU is 160 KiB) and, for a batch whose shape
// summary exceeds it, the capped LDS slice (2 waves per CU) plus the global-table launch's HBM budget.
constexpr int64_t kLdsBudget = 160 * 1024;
constexpr int64_t kLdsCapped = 80 * 1024;
constexpr int64_t kGlobalTableBudget = int64_t(2) << 30;
constexpr int kMaxR1 = 1 << 20;  // the screen rejects W >= 1e6 anyway

struct GenShape {
    int mmax, r1, tab, tab_kc;
};

// LDS shape of the general kernel's launches for a batch summary (full when it fits the budget).
GenShape lds_shape(const GenShape &full, bool *big) {
    const int64_t need = std::max(slice_bytes_for(full.mmax, full.r1, full.tab, 0),
                                  slice_bytes_for(full.mmax, full.r1, 0, full.tab_kc));
    *big = need > kLdsBudget;
    if (!*big) return full;
    GenShape g;
    g.mmax = std::min(full.mmax, kK1MaxM);
    g.r1 = std::min(full.r1, 128);
    while (true) {
        const int t = g.mmax * odd_stride(g.r1);
        g.tab = full.tab > 0 ? std::min(full.tab, t) : 0;
        g.tab_kc = full.tab_kc > 0 ? std::min(full.tab_kc, t) : 0;
        const int64_t b = std::max(slice_bytes_for(g.mmax, g.r1, std::max(g.tab, 1), 0),
                                   slice_bytes_for(g.mmax, g.r1, 0, g.tab_kc));
        if (b <= kLdsCapped || g.r1 <= 8) break;
        g.r1 = (g.r1 + 1) / 2;
    }
    g.tab = std::max(g.tab, 1);
    return g;
}

// Device-side ordering across streams: the verdict bytes, the hand-back flag and the fleet scratch
// are per context, so a launch that uses them on another stream than the previous such launch
// waits for everything enqueued on that stream so far (same stream: stream order already
// serialises them). A launch that touches none of them (the fused sweep's register launch when it
// needs no table launch behind it) neither waits nor is waited for: independent batches on two
// streams overlap on the device.
int order_after_previous(Ctx *ctx, hipStream_t s) {
    if (ctx->have_last && ctx->last_stream != s) {
        HIP_TRY(hipEventRecord(ctx->ev_order, ctx->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, ctx->ev_order, 0));
    }
    ctx->last_stream = s;
    ctx->have_last = true;
    return HALDA_OK;
}

// A grow-only device buffer (a stream's scratch slot, see Ctx::SweepSlot; the context's staging scratch):
// grown to hold `need` bytes at *buf.
template <class T>
int grow(T **buf, size_t *bytes, size_t need) {
    need = (need + 255) & ~size_t(255);
    if (need > *bytes) {
        if (*buf) HIP_TRY(hipFree(*buf));  // hipFree waits for the device
        *buf = nullptr;
        *bytes = 0;
        HIP_TRY(hipMalloc(buf, need));
        *bytes = need;
    }
    return HALDA_OK;
}

// The host entries' staging (layouts: halda_stage.hpp): the context's scratch grown to `bytes`, then one
// copy per array straight between the caller's memory and the scratch (a DMA where the caller's is
// page-locked, halda_host_alloc). An empty array is skipped, on the way back an absent one too.
int ensure_scratch(Ctx *c, size_t bytes) { return grow(&c->scratch, &c->scratch_bytes, bytes); }

int upload(char *base, size_t o, const void *src, size_t bytes, hipStream_t s) {
    if (bytes) HIP_TRY(hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, s));
    return HALDA_OK;
}

int upload(char *base, const stage::TableLayout &t, const halda_fleets &F, hipStream_t s) {
    int rc = upload(base, t.dev_off, F.dev_off, 8 * (t.nf + 1), s);
    if (rc == HALDA_OK) rc = upload(base, t.os_class, F.os_class, t.nd, s);
    if (rc == HALDA_OK) rc = upload(base, t.flags, F.flags, t.nd, s);
    for (int a = 0; a < stage::kFields && rc == HALDA_OK; ++a)
        rc = upload(base, t.field[a], F.*stage::kField[a], 8 * t.nd, s);
    return rc;
}

int upload(char *base, const stage::ItemsLayout &t, const halda_subfleets &I, hipStream_t s) {
    int rc = upload(base, t.parent, I.parent, 4 * t.n, s);
    if (rc == HALDA_OK) rc = upload(base, t.sub_off, I.sub_off, 8 * (t.n + 1), s);
    if (rc == HALDA_OK) rc = upload(base, t.sub_idx, I.sub_idx, 4 * t.tot, s);
    return rc;
}

int upload(char *base, const stage::TripleLayout &t, hipStream_t s) {
    int rc = HALDA_OK;
    for (int a = 0; a < 3 && rc == HALDA_OK; ++a)
        if (t.host[a]) rc = upload(base, t.off[a], t.host[a], 4 * t.count, s);
    return rc;
}

template <size_t N>
int download(const std::array<stage::Copy, N> &copies, const char *base, hipStream_t s) {
    for (const stage::Copy &k : copies)
        if (k.host && k.bytes) HIP_TRY(hipMemcpyAsync(k.host, base + k.off, k.bytes, hipMemcpyDeviceToHost, s));
    return HALDA_OK;
}

// The fused sweep's scratch slot for stream s with room for nf fleet flags (see Ctx::SweepSlot).
int sweep_slot(Ctx *c, hipStream_t s, int64_t nf, Ctx::SweepSlot **out) {
    Ctx::SweepSlot *slot = nullptr;
    for (auto &x : c->sws)
        if (x.used && x.stream == s) slot = &x;
    if (!slot) {
        for (auto &x : c->sws)
            if (!slot || (!x.used && slot->used) || (x.used == slot->used && x.tick < slot->tick)) slot = &x;
        if (slot->used) {  // taken over from another stream: after everything enqueued there so far
            HIP_TRY(hipEventRecord(slot->ev, slot->stream));
            HIP_TRY(hipStreamWaitEvent(s, slot->ev, 0));
        } else {
            HIP_TRY(hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming));
            HIP_TRY(hipMalloc(&slot->hb, 256));
            HIP_TRY(hipMemsetAsync(slot->hb, 0, 256, s));
            slot->used = true;
        }
        slot->stream = s;
    }
    slot->tick = ++c->sws_tick;
    if (nf > 0) {
        const int rc = grow(&slot->fflag, &slot->fflag_bytes, size_t(nf));
        if (rc != HALDA_OK) return rc;
    }
    *out = slot;
    return HALDA_OK;
}

int launch(Ctx *ctx, const halda_batch &in, const halda_result &out, hipStream_t stream,
           const uint8_t *settled = nullptr) {
    if (in.n_inst <= 0) return HALDA_OK;
    if (in.max_cols < 1 || in.max_R1 < 1 || in.max_tab < 0 || in.max_tab_kc < 0)
        return fail(HALDA_E_ARG, "halda_batch shape summary (max_cols/max_R1/max_tab/max_tab_kc) not set");
    if (in.max_R1 > kMaxR1) return fail(HALDA_E_ARG, "max_R1 > 2^20 (W - sum lb(w) must be < 2^20)");
    const int mmax = (in.max_cols - 1) / 7 + 1;
    // table sizes in doubles with the odd row stride used on chip
    // M * RS <= M * (R + 1) + M: the odd row stride costs at most one double per device
    const int64_t tab = std::max<int64_t>(1, in.max_tab > 0 ? int64_t(in.max_tab) + mmax : 0);
    const int64_t tab_kc = in.max_tab_kc > 0 ? int64_t(in.max_tab_kc) + mmax : 0;
    if (tab > (1 << 27) || tab_kc > (1 << 27)) return fail(HALDA_E_ARG, "table summary out of range (> 2^27)");
    const GenShape full{mmax, in.max_R1, int(tab), int(tab_kc)};
    bool big = false;
    const GenShape ls = lds_shape(full, &big);
    const size_t n = size_t(in.n_inst);
    // the verdict bytes and the hand-back flag are this stream's (its scratch slot): launches on other
    // streams need no ordering with this one; only the global tables of the big launch are shared
    Ctx::SweepSlot *slot = nullptr;
    {
        int rc = sweep_slot(ctx, stream, 0, &slot);
        if (rc == HALDA_OK) rc = grow(&slot->cls, &slot->cls_bytes, n);
        if (rc != HALDA_OK) return rc;
    }
    // global tables of the big launch: one slice per resident wave, grown on demand
    int64_t gstride = 0;
    int ggrid = 0;
    if (big) {
        gstride = (make_slice(full.mmax, full.r1, full.tab, full.tab_kc).total + 255) & ~int64_t(255);
        int per_cu = 0;
        HIP_TRY(ctx->occupancy(reinterpret_cast<const void *>(halda_solve_big_kernel), 0, &per_cu));
        ggrid = int(std::max<int64_t>(
            1, std::min<int64_t>({int64_t(ctx->cus) * per_cu, int64_t(n), kGlobalTableBudget / gstride})));
        const size_t need = size_t(gstride) * size_t(ggrid);
        if (need > ctx->gtab_bytes) {
            if (ctx->gtab) HIP_TRY(hipFree(ctx->gtab));
            ctx->gtab = nullptr;
            ctx->gtab_bytes = 0;
            HIP_TRY(hipMalloc(&ctx->gtab, need));
            ctx->gtab_bytes = need;
        }
    }
    if (big) {
        const int rc = order_after_previous(ctx, stream);
        if (rc != HALDA_OK) return rc;
    }
    uint8_t *cls = slot->cls;
    int *hb_flag = slot->hb;
    int *gen_flag = slot->hb + 16;  // its own 64 B of the slot's flag block
    const int launch_id = ++ctx->launch_id;  // tags this launch's flags: k = 1 hand-backs, k > 1 work (no reset)
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev0, stream));
    const int64_t lds1 = make_k1_slice(std::min(mmax, kK1MaxM)).total;
    if (settled && ctx->fused_screen) {
        // a settled batch: no screen launch -- the persistent k = 1 kernel writes the settled instances'
        // outputs and screens every other instance on its way (halda_solve_k1_settled_kernel)
        ctx->fused_last = true;
        int per_cu = 0;
        HIP_TRY(ctx->occupancy(reinterpret_cast<const void *>(halda_solve_k1_settled_kernel), lds1, &per_cu));
        const int grid = int(std::max<int64_t>(1, std::min<int64_t>(int64_t(ctx->cus) * per_cu, in.n_inst)));
        hipLaunchKernelGGL(halda_solve_k1_settled_kernel, dim3(grid), dim3(64), size_t(lds1), stream, in, out, cls,
                           mmax, hb_flag, launch_id, settled, gen_flag, in.max_R1, int(tab), int(tab_kc));
        HIP_TRY(hipGetLastError());
    } else {
        ctx->fused_last = false;
        // screen kernel (8 instances per wave), then a persistent k = 1 kernel
        const int64_t screen_waves = (int64_t(in.n_inst) + kScreenPer - 1) / kScreenPer;
        hipLaunchKernelGGL(halda_screen_kernel, dim3(unsigned((screen_waves + 3) / 4)), dim3(256), 0, stream, in, out,
                           cls, mmax, in.max_R1, int(tab), int(tab_kc), settled, gen_flag, launch_id);
        HIP_TRY(hipGetLastError());
        if (ctx->timing) HIP_TRY(hipEventRecord(ctx->evk, stream));
        int per_cu = 0;
        HIP_TRY(ctx->occupancy(reinterpret_cast<const void *>(halda_solve_k1_kernel), lds1, &per_cu));
        const int grid = int(std::max<int64_t>(1, std::min<int64_t>(int64_t(ctx->cus) * per_cu, in.n_inst)));
        hipLaunchKernelGGL(halda_solve_k1_kernel, dim3(grid), dim3(64), size_t(lds1), stream, in, out, cls, mmax,
                           hb_flag, launch_id);
        HIP_TRY(hipGetLastError());
    }
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->evs, stream));
    // general kernel, two launches with their own LDS slices: k > 1 instances (tables of the k > 1
    // shape only), then k = 1 instances of fleets wider than kK1MaxM devices and the fast path's
    // hand-backs (k = 1 tables). The first runs only when the shape summary admits k > 1 instances;
    // the second is gated on the hand-back flag unless wide k = 1 fleets are possible. A batch whose
    // summary exceeds the LDS budget gets capped slices and a third launch on global-memory tables
    // for the instances beyond them.
    const bool wide = (in.max_cols - 1) / 7 > kK1MaxM;
    if (ls.tab_kc > 0) {
        const int64_t lds_kc = slice_bytes_for(ls.mmax, ls.r1, 0, ls.tab_kc);
        int per_cu = 0;
        HIP_TRY(ctx->occupancy(reinterpret_cast<const void *>(halda_solve_kernel), lds_kc, &per_cu));
        const int grid = int(std::max<int64_t>(1, std::min<int64_t>(int64_t(ctx->cus) * per_cu, in.n_inst)));
        // gated on the screen's flag: a batch whose k > 1 instances were all settled by the screen (C3:
        // every k > 1 is bound-infeasible) leaves this launch nothing to do
        hipLaunchKernelGGL(halda_solve_kernel, dim3(grid), dim3(64), size_t(lds_kc), stream, in, out, cls, ls.mmax,
                           ls.r1, 0, ls.tab_kc, static_cast<const int *>(gen_flag), launch_id, 1, int(CLS_GEN));
        HIP_TRY(hipGetLastError());
    }
    {
        const int64_t lds_k1 = slice_bytes_for(ls.mmax, ls.r1, ls.tab, 0);
        int per_cu = 0;
        HIP_TRY(ctx->occupancy(reinterpret_cast<const void *>(halda_solve_kernel), lds_k1, &per_cu));
        const int64_t cap = wide ? int64_t(ctx->cus) * per_cu : int64_t(ctx->cus);
        const int grid = int(std::max<int64_t>(1, std::min<int64_t>(cap, in.n_inst)));
        hipLaunchKernelGGL(halda_solve_kernel, dim3(grid), dim3(64), size_t(lds_k1), stream, in, out, cls, ls.mmax,
                           ls.r1, ls.tab, 0, static_cast<const int *>(hb_flag), launch_id, int(!wide),
                           int(CLS_GEN1));
        HIP_TRY(hipGetLastError());
    }
    if (big) {
        hipLaunchKernelGGL(halda_solve_big_kernel, dim3(unsigned(ggrid)), dim3(64), 0, stream, in, out, cls,
                           full.mmax, full.r1, full.tab, full.tab_kc, static_cast<unsigned char *>(ctx->gtab),
                           gstride);
        HIP_TRY(hipGetLastError());
    }
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev1, stream));
    if (ctx->timing) ctx->timed = true;
    return HALDA_OK;
}

// Fused k-sweep (halda_sweep_kernel): one register-only launch over every fleet, then the table
// launch for the fleets it flagged (gated on the hand-back flag); a batch whose k > 1 / wide
// fleets need tables from the start gets the table launch only (LDS slice), or, beyond the LDS
// budget, the register launch plus the global-table launch.
constexpr int kSweepSmallBatch = 64;

// The fused sweep's launch sequence for one batch shape, derived from the shapes alone (no HIP call):
// which kernels, their grids and LDS slices, and the kernel arguments but for the per-launch scratch
// fields (fflag, hb_flag, launch_id, want), which run_sweep fills. sweep_fleets plans and runs in one
// go; a prepared plan (halda_fleets_plan_create) is planned once and run per launch.
enum SweepKind { kRegAlone, kRegGated, kRegBig, kTablesAlone, kSegGated, kKslotGated };

struct SweepPlan {
    SweepArgs A;
    SlotArgs SA;
    SweepKind kind;
    bool scratch;      // per-fleet flags / hand-back flag of the stream's slot in use
    int nf;
    int64_t lds;       // the first launch's dynamic LDS (k-slot / segment / table kernel)
    int64_t slice;     // the table kernel's LDS slice
    unsigned grid1;    // the first launch's grid
    unsigned block1;   // its workgroup size
    unsigned grid2;    // the gated second launch's grid (0: none)
    const void *fn1;   // first kernel (for the occupancy / LDS attribute)
};

lrec::Record sweep_record(SweepKind k) {
    switch (k) {
        case kRegAlone: return lrec::Record::reg_alone;
        case kTablesAlone: return lrec::Record::tables_alone;
        case kSegGated: return lrec::Record::seg_then_tables;
        case kKslotGated: return lrec::Record::kslot_then_tables;
        default: return lrec::Record::reg_then_tables;  // kRegGated, kRegBig
    }
}

int plan_sweep(Ctx *c, const halda_model &model, const halda_fleets &F, const int32_t *kh, int n_k,
               const halda_fleet_result &out, SweepPlan *P) {
    const int nf = F.n_fleets;
    int64_t r1_k1 = 0, r1_kc = 0;
    for (int j = 0; j < n_k; ++j) {
        const int64_t r1 = int64_t(model.L / kh[j]) - F.min_devices + 1;
        if (kh[j] == 1) r1_k1 = std::max(r1_k1, r1);
        else r1_kc = std::max(r1_kc, r1);
    }
    const int mmax = F.max_devices;
    const int64_t r1max = std::max<int64_t>(1, std::max(r1_k1, r1_kc));
    // table sizes in doubles (odd row stride: at most one extra double per device)
    const int64_t tab = r1_k1 > 0 ? int64_t(mmax) * r1_k1 + mmax : 1;
    const int64_t tab_kc = r1_kc > 0 ? int64_t(mmax) * r1_kc + mmax : 0;
    if (r1max > kMaxR1 || tab > (1 << 27) || tab_kc > (1 << 27))
        return fail(HALDA_E_ARG, "fleet shape out of range: (L / k_min - min_devices + 1) * max_devices > 2^27");
    const bool tables_first = tab_kc > 0 || mmax > kK1MaxM;
    const int64_t slice = make_slice(mmax, int(r1max), int(tab), int(tab_kc)).total;
    const bool fits = slice <= kLdsBudget;
    // fleets of <= 16 devices needing k > 1 tables: the lane-segment launch (four fleets per wave),
    // then the table launch for what it flagged
    const int64_t seg_lds = seg_slice_bytes(mmax, int(tab_kc)) * (64 / kSegLanes);
    // k-slot launch (preferred): the same fleets, one wave per (four fleets, open k)
    SlotArgs SA = {};
    int64_t kslot_lds = 0;
    for (int j = 0; j < n_k && SA.n_slot < kMaxSlots; ++j) {
        const int W = model.L / kh[j];
        if (!(W < 1000000) || W < F.min_devices) continue;  // settled for every fleet of the batch
        const int q = SA.n_slot++;
        SA.j[q] = j;
        SA.r1[q] = W - F.min_devices + 1;
        // a fleet of M >= min_devices devices has R + 1 <= r1 rows of odd stride <= odd_stride(r1)
        SA.tab[q] = kh[j] > 1 && W > F.min_devices ? mmax * odd_stride(SA.r1[q]) : 0;
        SA.off[q] = int(kslot_lds);
        kslot_lds += (64 / kSegLanes) * kslot_slice_bytes(mmax, SA.tab[q]);
    }
    bool kslot_all = true;  // every k that is open for some fleet has a slot
    for (int j = 0, q = 0; j < n_k; ++j) {
        const int W = model.L / kh[j];
        if (!(W < 1000000) || W < F.min_devices) continue;
        kslot_all = kslot_all && q < SA.n_slot && SA.j[q] == j;
        ++q;
    }
    // region 0 holds, one after another, the device records (read before any table is written), the
    // tables, and the pick area (written after the last table read): as large as the largest of them
    const int64_t pick_bytes = int64_t(64 / kSegLanes) * SA.n_slot * int64_t(sizeof(SlotPick));
    kslot_lds = std::max<int64_t>({kslot_lds, pick_bytes, int64_t(sizeof(KslotRecs))});
    SA.pick_off = 0;
    SA.rec_off = 0;
    // the threshold scan of the slot with the largest tables (C2: k = 2, the workgroup's critical path)
    // is split over kslot_split waves: the slot's own and, first thing after the tables, the waves of
    // the lightest other slots (no tables: k = 1 / W = M; else the smallest tables) -- an extra wave
    // only when there is no other slot
    SA.helper = -1;
    SA.n_parts = 0;
    if (c->kslot_split >= 2) {
        int r1 = 0;
        for (int q = 0; q < SA.n_slot; ++q)
            if (SA.tab[q] > 0 && SA.r1[q] > r1) {
                r1 = SA.r1[q];
                SA.helper = q;
            }
    }
    if (SA.helper >= 0) {
        // helpers: the lightest other slots (no tables, then the smallest; ties: the later slot)
        int used = 0;
        for (int h = 0; h < c->kslot_split - 1; ++h) {
            int pick = -1, light = 1 << 30;
            for (int q = 0; q < SA.n_slot; ++q) {
                const int work = SA.tab[q] > 0 ? SA.r1[q] : 0;
                bool taken = q == SA.helper;
                for (int u = 0; u < used; ++u) taken = taken || SA.part_wave[u] == q;
                if (!taken && work <= light) {
                    light = work;
                    pick = q;
                }
            }
            if (pick < 0) break;
            SA.part_wave[used++] = pick;
        }
        if (used == 0) {  // no other slot: one extra wave takes part 2
            if (SA.n_slot < kMaxSlots) SA.part_wave[used++] = SA.n_slot;
            else SA.helper = -1;
        }
        SA.n_parts = used + 1;
    }
    // the leaf checks of an optimistic part 1 (kslot_check): the table slot with the smallest tables
    // other than the split one (it ends its own solve first), else the other no-table slot, else the
    // helper itself
    SA.check_wave = -1;
    if (SA.helper >= 0) {
        SA.check_wave = SA.part_wave[0];
        int best = 1 << 30;
        for (int q = 0; q < SA.n_slot; ++q) {
            if (q == SA.helper || q == SA.part_wave[0]) continue;
            const int work = SA.tab[q] > 0 ? SA.r1[q] : (1 << 20);  // a no-table slot: its k = 1 greedy
            if (work < best) {
                best = work;
                SA.check_wave = q;
            }
        }
    }
    SA.crit_w4 = c->kslot_crit_w4;
    SA.cut8 = c->kslot_cut8;
    SA.opt = c->kslot_opt ? 1 : 0;
    kslot_lds = align16(kslot_lds);
    SA.split_off = int(kslot_lds);
    if (SA.helper >= 0) kslot_lds += int64_t(64 / kSegLanes) * int64_t(sizeof(SplitArea));
    kslot_lds = align16(kslot_lds);
    kslot_lds += c->kslot_pad;
    const bool kslot = c->seg_sweep && c->kslot_sweep && fits && mmax <= kSegLanes && tab_kc > 0 && kslot_all &&
                       SA.n_slot >= 1 && nf > kSweepSmallBatch && kslot_lds <= kLdsBudget;
    const bool seg = !kslot && c->seg_sweep && fits && mmax <= kSegLanes && n_k <= kSegLanes && tab_kc > 0 &&
                     nf > kSweepSmallBatch && seg_lds <= kLdsBudget;
    // small batches (a single halda_solve) take one launch: the register kernel when it needs no table
    // launch behind it, else the table kernel alone
    const bool small_tables = nf <= kSweepSmallBatch && r1_k1 > kDpLanes;
    const bool reg_mode = !seg && !kslot && !(fits && (tables_first || small_tables));
    // the register launch flags k > 1 / wide fleets (tables_first) and k = 1 greedy fallbacks with
    // R + 1 > kDpLanes; the others it solves itself (k1_dp), so no table launch is needed without them
    const bool gate = tables_first || r1_k1 > kDpLanes;
    SweepPlan &p = *P;
    p = SweepPlan{};
    p.nf = nf;
    p.slice = slice;
    p.scratch = !(reg_mode && !gate);
    SweepArgs &A = p.A;
    static_cast<halda_model &>(A.Mo) = model;
    A.Mo.bvo = model_bvo(model);
    A.F = F;
    for (int j = 0; j < n_k; ++j) {
        A.ks[j] = kh[j];
        A.Ws[j] = kh[j] != 0 ? model.L / kh[j] : 0;
    }
    A.n_k = n_k;
    A.out = FleetOut(out);
    A.outs = (out.obj_by_k ? kOutObk : 0) | (out.status ? kOutSt : 0) | (out.x ? kOutX : 0) | (out.c ? kOutC : 0) |
             (c->x_zero ? kOutXZ : 0);
    A.x_off = out.x_off;
    A.xstride = 7 * int64_t(std::max(mmax, 1)) + 1;
    A.mmax = mmax;
    A.uM = F.min_devices == F.max_devices ? F.max_devices : 0;
    A.k1dp = c->k1_force_dp ? 1 : 0;
    A.r1max = int(r1max);
    A.tab = int(tab);
    A.tab_kc = int(tab_kc);
    p.SA = SA;
    const unsigned cap_cus = unsigned(std::min<int64_t>(c->cus, nf));
    if (kslot) {
        p.kind = kKslotGated;
        p.fn1 = reinterpret_cast<const void *>(halda_sweep_kslot_kernel);
        p.lds = kslot_lds;
        p.grid1 = unsigned((int64_t(nf) + 64 / kSegLanes - 1) / (64 / kSegLanes));
        p.block1 = unsigned(64 * kslot_waves(SA));
        p.grid2 = cap_cus;
    } else if (seg) {
        p.kind = kSegGated;
        p.fn1 = reinterpret_cast<const void *>(halda_sweep_seg_kernel);
        p.lds = seg_lds;
        int per_cu = 0;
        HIP_TRY(c->occupancy(p.fn1, seg_lds, &per_cu));
        const int64_t nw = (int64_t(nf) + 64 / kSegLanes - 1) / (64 / kSegLanes);
        p.grid1 = unsigned(std::max<int64_t>(1, std::min<int64_t>(int64_t(c->cus) * per_cu, nw)));
        p.block1 = 64;
        p.grid2 = cap_cus;
    } else if (fits && (tables_first || small_tables)) {
        // small batches (a single halda_solve): one launch with the table slice instead of two
        p.kind = kTablesAlone;
        p.fn1 = reinterpret_cast<const void *>(halda_sweep_tables_kernel);
        p.lds = slice;
        int per_cu = 0;
        HIP_TRY(c->occupancy(p.fn1, slice, &per_cu));
        p.grid1 = unsigned(std::max<int64_t>(1, std::min<int64_t>(int64_t(c->cus) * per_cu, nf)));
        p.block1 = 64;
    } else {
        p.fn1 = reinterpret_cast<const void *>(halda_sweep_kernel);
        p.grid1 = unsigned((nf + kSweepWavesPerBlock - 1) / kSweepWavesPerBlock);
        p.block1 = 64 * kSweepWavesPerBlock;
        if (!gate) {
            p.kind = kRegAlone;
        } else if (fits) {  // flagged fleets are rare (fast-path fallbacks): one wave per CU is plenty
            p.kind = kRegGated;
            int per_cu = 0;
            HIP_TRY(c->occupancy(reinterpret_cast<const void *>(halda_sweep_tables_kernel), slice, &per_cu));
            p.grid2 = unsigned(std::max<int64_t>(1, std::min<int64_t>(tables_first ? int64_t(c->cus) * per_cu
                                                                                   : int64_t(c->cus), nf)));
        } else {
            p.kind = kRegBig;
            A.gstride = (slice + 255) & ~int64_t(255);
            int per_cu = 0;
            HIP_TRY(c->occupancy(reinterpret_cast<const void *>(halda_sweep_big_kernel), 0, &per_cu));
            p.grid2 = unsigned(std::max<int64_t>(
                1, std::min<int64_t>({int64_t(c->cus) * per_cu, int64_t(nf), kGlobalTableBudget / A.gstride})));
        }
    }
    if (p.kind == kKslotGated) {
        int per_cu = 0;
        HIP_TRY(c->occupancy(p.fn1, p.lds, &per_cu));
        if (std::getenv("HALDA_DEBUG_PLAN")) {  // diagnostic: the k-slot launch's LDS and residency
            int steps_cu = 0;
            (void)c->ensure_lds(reinterpret_cast<const void *>(halda_sweep_kslot_steps_kernel), p.lds);
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &steps_cu, reinterpret_cast<const void *>(halda_sweep_kslot_steps_kernel), int(p.block1),
                size_t(p.lds));
            std::fprintf(stderr, "halda plan: k-slot lds %lld B, block %u, per CU %d (steps kernel %d)\n",
                         (long long)p.lds, p.block1, per_cu, steps_cu);
        }
    }
    if (p.kind == kKslotGated || p.kind == kSegGated)
        HIP_TRY(c->occupancy(reinterpret_cast<const void *>(halda_sweep_tables_kernel), slice, nullptr));
    return HALDA_OK;
}

// An entry's first step on the GPU: the context's device made current (only when it is not), and the caller's
// stream, or the context's own for NULL.
int enter(Ctx *c, void *stream, hipStream_t *s) {
    int cur_dev = -1;
    if (hipGetDevice(&cur_dev) != hipSuccess || cur_dev != c->device) HIP_TRY(hipSetDevice(c->device));
    *s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return HALDA_OK;
}

// ---- what every launch of a fused-sweep kernel shares (the record itself: halda_launch.hpp)
// The per-launch fields of a plan's arguments: the scratch in use (none: the context's hand-back flag, never
// written), a fresh launch id, the first pass.
void stamp(Ctx *c, SweepArgs &A, uint8_t *fflag, int *hb_flag) {
    A.fflag = fflag;
    A.hb_flag = hb_flag;
    A.launch_id = ++c->launch_id;
    A.want = 0;
}

// From here on the context's last timed sequence and lowered batch are no longer the previous call's.
void forget_last(Ctx *c) {
    c->fleet_timed = false;
    c->have_lowered = false;
}

// A family's single launch, step one: arguments stamped (nothing flags, nothing is handed back), the last
// record forgotten. What the family must still look up (occupancy, an LDS limit) comes between this and launch_one.
void begin_one(Ctx *c, SweepArgs &A) {
    stamp(c, A, nullptr, c->hb_flag);
    forget_last(c);
}

int launched() {
    HIP_TRY(hipGetLastError());
    return HALDA_OK;
}

// The end of a timed sequence: evf1, and what ran.
int finish(Ctx *c, hipStream_t s, lrec::Record r) {
    if (c->timing) {
        HIP_TRY(hipEventRecord(c->evf1, s));
        c->fleet_timed = true;
    }
    c->fleet_record = r;
    return HALDA_OK;
}

// Step two: evf0, the family's kernel (`enqueue` launches it and answers its status), evf1, the record and the
// family's route. An error leaves the route and the record as they were.
template <class Enqueue>
int launch_one(Ctx *c, hipStream_t s, lrec::Record r, lrec::Family family, int route, Enqueue &&enqueue) {
    if (c->timing) HIP_TRY(hipEventRecord(c->evf0, s));
    int rc = enqueue();
    if (rc == HALDA_OK) rc = finish(c, s, r);
    if (rc == HALDA_OK) c->knob[family].route = route;
    return rc;
}

// halda_set_<family>_path / halda_last_<family>_route (the admissible paths: lrec::kKnobRules)
int set_family_path(void *ctx, lrec::Family family, int path) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return fail(HALDA_E_ARG, "NULL ctx");
    if (const char *why = lrec::path_error(family, path)) return fail(HALDA_E_ARG, why);
    c->knob[family].path = path;
    return HALDA_OK;
}

int last_family_route(void *ctx, lrec::Family family, int *route) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !route) return fail(HALDA_E_ARG, "NULL ctx/route");
    *route = c->knob[family].route;
    return HALDA_OK;
}

// Enqueue a planned sweep on stream s: the stream's scratch slot (when the plan uses scratch), the
// first launch and the gated table launch behind it (global tables: after the previous launch on them).
int run_sweep(Ctx *c, SweepPlan &p, hipStream_t s) {
    SweepArgs &A = p.A;
    Ctx::SweepSlot *slot = nullptr;
    if (p.scratch) {
        const int rc = sweep_slot(c, s, p.nf, &slot);
        if (rc != HALDA_OK) return rc;
    }
    stamp(c, A, p.scratch ? slot->fflag : nullptr, p.scratch ? slot->hb : c->hb_flag);
    forget_last(c);
    if (p.lds > 0) HIP_TRY(Ctx::ensure_lds(p.fn1, p.lds));
    if (c->timing) HIP_TRY(hipEventRecord(c->evf0, s));
    switch (p.kind) {
        case kKslotGated:
            hipLaunchKernelGGL(halda_sweep_kslot_kernel, dim3(p.grid1), dim3(p.block1), size_t(p.lds), s, A, p.SA);
            break;
        case kSegGated:
            hipLaunchKernelGGL(halda_sweep_seg_kernel, dim3(p.grid1), dim3(p.block1), size_t(p.lds), s, A);
            break;
        case kTablesAlone:
            hipLaunchKernelGGL(halda_sweep_tables_kernel, dim3(p.grid1), dim3(p.block1), size_t(p.lds), s, A);
            break;
        default:
            hipLaunchKernelGGL(halda_sweep_kernel, dim3(p.grid1), dim3(p.block1), 0, s, A);
            break;
    }
    HIP_TRY(hipGetLastError());
    const bool two = p.kind == kKslotGated || p.kind == kSegGated || p.kind == kRegGated || p.kind == kRegBig;
    if (two) {
        if (c->timing) HIP_TRY(hipEventRecord(c->evfm, s));
        A.want = 1;  // the fleets flagged above, gated on the hand-back flag
        if (p.kind == kRegBig) {
            const size_t gneed = size_t(A.gstride) * size_t(p.grid2);
            if (gneed > c->gtab_bytes) {
                if (c->gtab) HIP_TRY(hipFree(c->gtab));
                c->gtab = nullptr;
                c->gtab_bytes = 0;
                HIP_TRY(hipMalloc(&c->gtab, gneed));
                c->gtab_bytes = gneed;
            }
            // the global tables are per context (not per stream slot: up to 2 GiB each), so this launch
            // runs after the previous user of them on another stream (a sweep's or launch()'s big launch)
            const int rc = order_after_previous(c, s);
            if (rc != HALDA_OK) return rc;
            A.gtab = static_cast<unsigned char *>(c->gtab);
            hipLaunchKernelGGL(halda_sweep_big_kernel, dim3(p.grid2), dim3(64), 0, s, A);
        } else {
            HIP_TRY(Ctx::ensure_lds(reinterpret_cast<const void *>(halda_sweep_tables_kernel), p.slice));
            hipLaunchKernelGGL(halda_sweep_tables_kernel, dim3(p.grid2), dim3(64), size_t(p.slice), s, A);
        }
        HIP_TRY(hipGetLastError());
    }
    return finish(c, s, sweep_record(p.kind));
}

// The last call's arguments and plan: a caller repeating a call on the same buffers (a single
// halda_solve's staging, a re-profiled stream) is not re-planned.
struct SweepKey {
    halda_model model;
    halda_fleets F;
    halda_fleet_result out;
    int32_t ks[64];
    int n_k, path_gen;
    bool x_zero;
};

int cached_plan(Ctx *c, const halda_model &model, const halda_fleets &F, const int32_t *kh, int n_k,
                const halda_fleet_result &out, SweepPlan **plan) {
    static thread_local SweepKey last_key;
    static thread_local SweepPlan last_plan;
    static thread_local uint64_t last_ctx = 0;  // Ctx::uid
    SweepKey k;
    std::memset(&k, 0, sizeof k);
    k.model = model;
    k.F = F;
    k.out = out;
    std::memcpy(k.ks, kh, sizeof(int32_t) * size_t(n_k));
    k.n_k = n_k;
    k.path_gen = c->path_gen;
    k.x_zero = c->x_zero;
    if (last_ctx != c->uid || std::memcmp(&k, &last_key, sizeof k) != 0) {
        last_ctx = 0;
        const int rc = plan_sweep(c, model, F, kh, n_k, out, &last_plan);
        if (rc != HALDA_OK) return rc;
        last_key = k;
        last_ctx = c->uid;
    }
    *plan = &last_plan;
    return HALDA_OK;
}

int sweep_fleets(Ctx *c, const halda_model &model, const halda_fleets &F, const int32_t *kh, int n_k,
                 const halda_fleet_result &out, hipStream_t s) {
    SweepPlan *p = nullptr;
    const int rc = cached_plan(c, model, F, kh, n_k, out, &p);
    if (rc != HALDA_OK) return rc;
    return run_sweep(c, *p, s);
}

// One fleet through the resident wave (halda_resident_kernel), synchronously: the plan's arguments into
// the mailbox, the wave (re)launched when no launch of it is running, seq bumped, ack awaited. The
// fleet's table and results are the caller's fine-grained pinned buffers (device addresses in A).
// *done = false when the plan is not a register-only sweep of one fleet, or when the wave gave no answer
// in time and was stopped (the caller launches the sweep itself; the resident path is off from then on).
// *retry = true when the wave could not even be stopped: its pinned buffer is retired (kept allocated,
// never reused) and the caller redoes the whole call on a fresh one.
constexpr uint32_t kResidentIdleTicks = 200000;  // 2 ms of the 100 MHz clock without a request

// Stop the resident wave and wait (at most `budget`) until it has left: true when it has (or none ran).
bool resident_stop(Ctx *c, std::chrono::milliseconds budget) {
    if (!c->rbox || !c->rlive) return true;
    __atomic_store_n(&c->rbox->stop, 1u, __ATOMIC_SEQ_CST);
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t q;
    while ((q = hipEventQuery(c->rdone)) == hipErrorNotReady) {
        if (std::chrono::steady_clock::now() - t0 > budget) return false;
        std::this_thread::yield();
    }
    c->rlive = false;
    __atomic_store_n(&c->rbox->stop, 0u, __ATOMIC_SEQ_CST);  // the next launch stays until told
    return true;
}

int resident_sweep(Ctx *c, const SweepPlan &p, bool *done, bool *retry) {
    *done = false;
    *retry = false;
    if (!c->resident || p.kind != kRegAlone || p.nf != 1 || p.A.uM <= 0 || p.A.uM > kK1MaxM || p.A.k1dp) return HALDA_OK;
    if (!c->rbox) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&c->rbox), sizeof(ResidentBox),
                              hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(static_cast<void *>(c->rbox), 0, sizeof(ResidentBox));
        HIP_TRY(hipHostGetDevicePointer(&c->rbox_dev, c->rbox, 0));
        HIP_TRY(hipStreamCreateWithFlags(&c->rstream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->rdone, hipEventDisableTiming));
        c->rseq = 0;
    }
    ResidentBox *box = c->rbox;
    SweepArgs A = p.A;
    stamp(c, A, nullptr, c->hb_flag);
    std::memcpy(static_cast<void *>(&box->req), &A, sizeof A);
    auto launch = [&](uint32_t last) -> int {
        ResidentArgs R;
        R.box = static_cast<ResidentBox *>(c->rbox_dev);
        R.last = last;
        R.idle_ticks = kResidentIdleTicks;
        hipLaunchKernelGGL(halda_resident_kernel, dim3(1), dim3(64), 0, c->rstream, R);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->rdone, c->rstream));
        c->rlive = true;
        return HALDA_OK;
    };
    if (!c->rlive || hipEventQuery(c->rdone) == hipSuccess) {
        const int rc = launch(c->rseq);
        if (rc != HALDA_OK) return rc;
    }
    const uint32_t want = ++c->rseq;
    // after the request (x86: stores in order); the fault-injection mode never posts it
    if (!c->resident_drop) __atomic_store_n(&box->seq, want, __ATOMIC_SEQ_CST);
    // the answer; a wave that left (idle timeout) between its last poll and this request is relaunched
    const auto t0 = std::chrono::steady_clock::now();
    const auto limit = c->resident_drop ? std::chrono::milliseconds(20) : std::chrono::milliseconds(5000);
    for (uint64_t spin = 1;; ++spin) {
        if (__atomic_load_n(&box->ack, __ATOMIC_ACQUIRE) == want) break;
        if ((spin & 255) == 0) {
            if (hipEventQuery(c->rdone) == hipSuccess && __atomic_load_n(&box->ack, __ATOMIC_ACQUIRE) != want) {
                const int rc = launch(want - 1);
                if (rc != HALDA_OK) return rc;
            }
            if (std::chrono::steady_clock::now() - t0 > limit) {
                // no answer: never again on this context. The wave (or a late launch of it) still sees
                // request `want` pending and would write its results into the pinned buffer later, so it
                // is stopped and awaited before that buffer is touched again; then this call launches.
                c->resident = false;
                if (resident_stop(c, std::chrono::milliseconds(5000))) return HALDA_OK;
                c->retired.push_back(c->pinned);  // still the wave's: keep it allocated, never reuse it
                c->pinned = nullptr;
                c->pinned_dev = nullptr;
                c->pinned_bytes = 0;
                *retry = true;
                return HALDA_OK;
            }
        }
    }
    *done = true;
    return HALDA_OK;
}

// ---------------------------------------------------------------- latency mode over RCCL
// One process per GPU, the ranks of an RCCL communicator: rank r sweeps the k-candidates
// ks[r], ks[r + world], ... of every fleet (halda_sweep_* on its own GPU), then the ranks agree on each
// fleet's best k with the reference's rule -- the smallest obj_value, ties to the smallest k
// (halda_p_solver.py:407) -- by three all-reduces over xGMI: MIN of obj_value, MIN of the k that
// reaches it, SUM of (w, n) where only the owner of that k contributes (the ranks' k's are disjoint),
// plus MIN / MAX of the per-k objectives / statuses when requested. Kernels between them turn one
// reduction's output into the next one's input on the device; nothing returns to the host.
__global__ __launch_bounds__(64) void halda_shard_kernel(int mode, int n_k, int n_sub, int rank, int world,
                                                         const int64_t *dev_off, halda_fleet_result sub,
                                                         halda_fleet_result out) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int64_t d0 = dev_off[f], d1 = dev_off[f + 1];
    if (mode == 0) {  // local results into the full layout, neutral elements elsewhere
        if (lane == 0) out.obj_value[f] = n_sub > 0 ? sub.obj_value[f] : kInf;
        for (int64_t d = d0 + lane; d < d1; d += 64) {
            out.w[d] = n_sub > 0 ? sub.w[d] : 0;
            out.n[d] = n_sub > 0 ? sub.n[d] : 0;
        }
        for (int j = lane; j < n_k; j += 64) {
            const bool own = j % world == rank;
            const int js = j / world;
            if (out.obj_by_k) out.obj_by_k[int64_t(f) * n_k + j] = own ? sub.obj_by_k[int64_t(f) * n_sub + js] : kInf;
            if (out.status) out.status[int64_t(f) * n_k + j] = own ? sub.status[int64_t(f) * n_sub + js] : INT32_MIN;
        }
    } else if (mode == 1) {  // after MIN(obj_value): the k this rank offers for the global minimum
        if (lane == 0) {
            const int bk = n_sub > 0 ? sub.best_k[f] : 0;
            out.best_k[f] = bk > 0 && sub.obj_value[f] == out.obj_value[f] ? bk : INT32_MAX;
        }
    } else {  // after MIN(k): only the owner keeps its (w, n) for the SUM
        const int bk = n_sub > 0 ? sub.best_k[f] : 0;
        const int kmin = out.best_k[f];
        if (bk != kmin || kmin == INT32_MAX)
            for (int64_t d = d0 + lane; d < d1; d += 64) out.w[d] = out.n[d] = 0;
    }
}

__global__ __launch_bounds__(256) void halda_shard_final_kernel(int nf, halda_fleet_result out) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < nf && out.best_k[f] == INT32_MAX) out.best_k[f] = 0;  // no rank has a feasible k
}

int nccl_fail(ncclResult_t r, const char *what) {
    return fail(HALDA_E_HIP, std::string(what) + ": " + ncclGetErrorString(r));
}
#define NCCL_TRY(expr)                                     \
    do {                                                   \
        ncclResult_t r_ = (expr);                          \
        if (r_ != ncclSuccess) return nccl_fail(r_, #expr); \
    } while (0)

// The steps of latency mode, shared by the RCCL entry (one rank: this process's) and the one-device
// emulation of `world` ranks (tests, bench): per rank the sub-sweep of its k's and halda_shard_kernel
// mode 0, all-reduce MIN obj_value, mode 1, all-reduce MIN best_k, mode 2, then (one RCCL group) SUM w,
// SUM n, MIN obj_by_k, MAX status, and the final kernel. `ar(field, count)` performs one all-reduce (or
// opens / closes the group) over the ranks' `o` arrays.
enum ShardField { kShObj, kShBestK, kShGroupStart, kShW, kShN, kShObk, kShSt, kShGroupEnd };

struct ShardRank {
    int rank = 0;
    halda_fleet_result o = {};    // this rank's copy of the full result
    halda_fleet_result sub = {};  // its sub-sweep's results (its k's only)
    std::vector<int32_t> mine;    // ks[rank], ks[rank + world], ...
};

constexpr int kEmuMaxWorld = 16;
struct EmuReduce {
    int world;
    int field;
    int64_t count;
    void *p[kEmuMaxWorld];
};

// One emulated all-reduce: element i of every virtual rank's buffer becomes the MIN / SUM / MAX over
// the ranks (the RCCL operation of that field), in place.
__global__ __launch_bounds__(256) void halda_emu_allreduce_kernel(EmuReduce E) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= E.count) return;
    if (E.field == kShObj || E.field == kShObk) {
        double m = static_cast<const double *>(E.p[0])[i];
        for (int r = 1; r < E.world; ++r) {
            const double v = static_cast<const double *>(E.p[r])[i];
            m = v < m ? v : m;
        }
        for (int r = 0; r < E.world; ++r) static_cast<double *>(E.p[r])[i] = m;
    } else {
        int32_t m = static_cast<const int32_t *>(E.p[0])[i];
        for (int r = 1; r < E.world; ++r) {
            const int32_t v = static_cast<const int32_t *>(E.p[r])[i];
            m = E.field == kShBestK ? (v < m ? v : m) : E.field == kShSt ? (v > m ? v : m) : m + v;
        }
        for (int r = 0; r < E.world; ++r) static_cast<int32_t *>(E.p[r])[i] = m;
    }
}

// Devices in the batch: n_fleets * M for one fleet size, else dev_off[n_fleets] read back (synchronous).
int shard_device_count(const halda_fleets &F, hipStream_t s, int64_t *nd) {
    const int64_t nf = F.n_fleets;
    *nd = nf * F.max_devices;
    if (F.min_devices != F.max_devices) {
        HIP_TRY(hipMemcpyAsync(nd, F.dev_off + nf, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return HALDA_OK;
}

template <class AR>
int shard_steps(Ctx *c, const halda_model &model, const halda_fleets &F, const int32_t *ks, int n_k, int world,
                std::vector<ShardRank> &R, hipStream_t s, AR &&ar) {
    const halda_fleet_result &out = R[0].o;
    if (out.x || out.c) return fail(HALDA_E_ARG, "halda_solve_fleets_sharded: x / c are not gathered (pass NULL)");
    if (!out.best_k || !out.obj_value || !out.w || !out.n) return fail(HALDA_E_ARG, "halda_fleet_result: NULL");
    const int64_t nf = F.n_fleets;
    if (nf <= 0) return HALDA_OK;
    if (n_k <= 0 || n_k > 1024) return fail(HALDA_E_ARG, "n_k must be in 1..1024");
    for (int j = 0; j < n_k; ++j)
        if (ks[j] < 1 || (j && ks[j] <= ks[j - 1])) return fail(HALDA_E_ARG, "ks must be ascending, unique, > 0");
    int64_t nd = 0;
    {
        const int rc = shard_device_count(F, s, &nd);
        if (rc != HALDA_OK) return rc;
    }
    // rank-local sub-sweep results in the context's shard scratch (one block per rank state)
    stage::Bump lay;
    std::vector<size_t> o_bk, o_obj, o_w, o_n, o_obk, o_st;
    for (auto &r : R) {
        r.mine.clear();
        for (int j = r.rank; j < n_k; j += world) r.mine.push_back(ks[j]);  // as halda_solve_distributed deals them
        const size_t nsub = std::max<size_t>(r.mine.size(), 1);
        o_bk.push_back(lay.take(4 * nf));
        o_obj.push_back(lay.take(8 * nf));
        o_w.push_back(lay.take(4 * size_t(nd)));
        o_n.push_back(lay.take(4 * size_t(nd)));
        o_obk.push_back(lay.take(8 * nf * nsub));
        o_st.push_back(lay.take(4 * nf * nsub));
    }
    {
        const int rc = grow(&c->shard, &c->shard_bytes, lay.off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = static_cast<char *>(c->shard);
    for (size_t i = 0; i < R.size(); ++i) {
        halda_fleet_result &sub = R[i].sub;
        sub = {};
        sub.best_k = reinterpret_cast<int32_t *>(base + o_bk[i]);
        sub.obj_value = reinterpret_cast<double *>(base + o_obj[i]);
        sub.w = reinterpret_cast<int32_t *>(base + o_w[i]);
        sub.n = reinterpret_cast<int32_t *>(base + o_n[i]);
        sub.obj_by_k = out.obj_by_k ? reinterpret_cast<double *>(base + o_obk[i]) : nullptr;
        sub.status = out.status ? reinterpret_cast<int32_t *>(base + o_st[i]) : nullptr;
    }
    {
        const int rc = order_after_previous(c, s);  // the shard scratch is per context
        if (rc != HALDA_OK) return rc;
    }
    for (auto &r : R)
        if (!r.mine.empty()) {
            const int rc = halda_solve_fleets(c, &model, &F, r.mine.data(), int32_t(r.mine.size()), &r.sub, s);
            if (rc != HALDA_OK) return rc;
        }
    auto modes = [&](int mode) -> int {
        for (auto &r : R) {
            hipLaunchKernelGGL(halda_shard_kernel, dim3(unsigned(nf)), dim3(64), 0, s, mode, int(n_k),
                               int(r.mine.size()), r.rank, world, F.dev_off, r.sub, r.o);
            HIP_TRY(hipGetLastError());
        }
        return HALDA_OK;
    };
    int rc = modes(0);
    if (rc == HALDA_OK) rc = ar(kShObj, size_t(nf));
    if (rc == HALDA_OK) rc = modes(1);
    if (rc == HALDA_OK) rc = ar(kShBestK, size_t(nf));
    if (rc == HALDA_OK) rc = modes(2);
    if (rc == HALDA_OK) rc = ar(kShGroupStart, 0);
    if (rc == HALDA_OK) rc = ar(kShW, size_t(nd));
    if (rc == HALDA_OK) rc = ar(kShN, size_t(nd));
    if (rc == HALDA_OK && out.obj_by_k) rc = ar(kShObk, size_t(nf) * n_k);
    if (rc == HALDA_OK && out.status) rc = ar(kShSt, size_t(nf) * n_k);
    if (rc == HALDA_OK) rc = ar(kShGroupEnd, 0);
    if (rc != HALDA_OK) return rc;
    for (auto &r : R) {
        hipLaunchKernelGGL(halda_shard_final_kernel, dim3(unsigned((nf + 255) / 256)), dim3(256), 0, s, int(nf), r.o);
        HIP_TRY(hipGetLastError());
    }
    return HALDA_OK;
}

}  // namespace

extern "C" {

int halda_version(void) { return HALDA_ABI_VERSION; }

int halda_last_error(char *buf, size_t len) {
    if (buf && len) std::snprintf(buf, len, "%s", g_err.c_str());
    return int(g_err.size());
}

int64_t halda_lds_bytes(int32_t max_cols, int32_t max_R1, int32_t max_tab, int32_t max_tab_kc) {
    if (max_R1 < 1 || max_R1 > kMaxR1) return -1;
    const int mmax = (max_cols - 1) / 7 + 1;
    const int64_t tab = std::max<int64_t>(1, max_tab > 0 ? int64_t(max_tab) + mmax : 0);
    const int64_t tab_kc = max_tab_kc > 0 ? int64_t(max_tab_kc) + mmax : 0;
    return std::max(slice_bytes_for(mmax, max_R1, int(tab), 0), slice_bytes_for(mmax, max_R1, 0, int(tab_kc)));
}

int halda_init(int device_ordinal, void **ctx_out) {
    if (!ctx_out) return fail(HALDA_E_ARG, "ctx is NULL");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(HALDA_E_NODEV, "no HIP device visible (libhalda needs an MI355X / gfx950)");
    if (device_ordinal < 0 || device_ordinal >= count)
        return fail(HALDA_E_NODEV, "device ordinal " + std::to_string(device_ordinal) + " out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(HALDA_E_NODEV, std::string("libhalda is built for gfx950, device is ") + prop.gcnArchName);
    HIP_TRY(hipSetDevice(device_ordinal));
    Ctx *c = new Ctx();
    c->device = device_ordinal;
    c->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipMalloc(&c->hb_flag, 256) != hipSuccess || hipMemset(c->hb_flag, 0, 256) != hipSuccess) {
        delete c;
        return fail(HALDA_E_HIP, "hand-back flag allocation failed");
    }
    const char *fp = std::getenv("HALDA_FLEETS_PATH");
    c->fleets_fused = !(fp && std::strcmp(fp, "csr") == 0);
    c->seg_sweep = !(fp && std::strcmp(fp, "wave") == 0);
    const char *hp = std::getenv("HALDA_HOST_PATH");  // diagnostic A/B of the small synchronous call
    c->host_copy = hp && std::strcmp(hp, "copy") == 0;
    const char *rs = std::getenv("HALDA_RESIDENT");
    c->resident = !(rs && std::strcmp(rs, "0") == 0);
    const char *fs = std::getenv("HALDA_FUSED_SCREEN");  // A/B: the screen launch before a settled batch's k = 1 kernel
    c->fused_screen = !(fs && std::strcmp(fs, "0") == 0);
    const char *kw = std::getenv("HALDA_KSLOT_CRIT_W4");  // diagnostic A/B of the critical slot's table share
    if (kw && std::atoi(kw) > 0) c->kslot_crit_w4 = std::atoi(kw);
    const char *kc8 = std::getenv("HALDA_KSLOT_CUT8");  // diagnostic A/B of the split scan's cut
    if (kc8 && std::atoi(kc8) >= 1 && std::atoi(kc8) <= 7) c->kslot_cut8 = std::atoi(kc8);
    const char *kp = std::getenv("HALDA_KSLOT_LDS_PAD");
    c->kslot_pad = kp ? std::max(0, std::atoi(kp)) : 0;
    const char *rt = std::getenv("HALDA_RESIDENT_TEST");
    c->resident_drop = rt && std::strcmp(rt, "drop") == 0;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->evs) != hipSuccess || hipEventCreate(&c->evk) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_host, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->evf0) != hipSuccess || hipEventCreate(&c->evf1) != hipSuccess ||
        hipEventCreate(&c->evfm) != hipSuccess) {
        halda_free(c);
        return fail(HALDA_E_HIP, "stream/event creation failed");
    }
    *ctx_out = c;
    return HALDA_OK;
}

int halda_resident_release(void *ctx) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return fail(HALDA_E_ARG, "null context");
    if (!resident_stop(c, std::chrono::milliseconds(5000)))
        return fail(HALDA_E_HIP, "resident solver: the wave did not leave within 5 s");
    return HALDA_OK;
}

int halda_host_alloc(size_t bytes, void **ptr) {
    if (!ptr || bytes == 0) return fail(HALDA_E_ARG, "halda_host_alloc: NULL ptr or zero bytes");
    *ptr = nullptr;
    HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    std::lock_guard<std::mutex> lock(g_host_mu);
    g_host_blocks.emplace_back(reinterpret_cast<uintptr_t>(*ptr), bytes);
    return HALDA_OK;
}

void halda_host_free(void *ptr) {
    if (!ptr) return;
    {
        std::lock_guard<std::mutex> lock(g_host_mu);
        for (size_t i = 0; i < g_host_blocks.size(); ++i)
            if (g_host_blocks[i].first == reinterpret_cast<uintptr_t>(ptr)) {
                g_host_blocks.erase(g_host_blocks.begin() + i);
                break;
            }
    }
    (void)hipHostFree(ptr);
}

void halda_free(void *ctx) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return;
    for (CtxHandle *h : c->handles) h->c = nullptr;  // plans / groups outliving the context fail cleanly
    c->handles.clear();
    if (c->rbox) {
        if (c->rlive) {  // the resident wave leaves at its next poll
            __atomic_store_n(&c->rbox->stop, 1u, __ATOMIC_SEQ_CST);
            (void)hipEventSynchronize(c->rdone);
        }
        (void)hipHostFree(c->rbox);
    }
    for (void *b : c->retired) (void)hipHostFree(b);  // the wave that held them has left (above)
    if (c->rdone) (void)hipEventDestroy(c->rdone);
    if (c->rstream) (void)hipStreamDestroy(c->rstream);
    (void)hipSetDevice(c->device);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->work) (void)hipFree(c->work);
    if (c->hb_flag) (void)hipFree(c->hb_flag);
    if (c->fleet_scratch) (void)hipFree(c->fleet_scratch);
    if (c->gtab) (void)hipFree(c->gtab);
    if (c->sub_tab) (void)hipFree(c->sub_tab);
    if (c->sel_buf) (void)hipFree(c->sel_buf);
    if (c->var_desc) (void)hipFree(c->var_desc);
    for (auto &x : c->sws) {
        if (x.fflag) (void)hipFree(x.fflag);
        if (x.cls) (void)hipFree(x.cls);
        if (x.hb) (void)hipFree(x.hb);
        if (x.ev) (void)hipEventDestroy(x.ev);
    }
    if (c->shard) (void)hipFree(c->shard);
    if (c->emu) (void)hipFree(c->emu);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->ev_host) (void)hipEventDestroy(c->ev_host);
    if (c->evf0) (void)hipEventDestroy(c->evf0);
    if (c->evf1) (void)hipEventDestroy(c->evf1);
    if (c->evfm) (void)hipEventDestroy(c->evfm);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->evs) (void)hipEventDestroy(c->evs);
    if (c->evk) (void)hipEventDestroy(c->evk);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int halda_solve_batch_device(void *ctx, const halda_batch *in, halda_result *out, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !in || !out) return fail(HALDA_E_ARG, "NULL ctx/in/out");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return launch(c, *in, *out, s);
}

int halda_solve_batch_device_settled(void *ctx, const halda_batch *in, halda_result *out, const uint8_t *settled,
                                     void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !in || !out) return fail(HALDA_E_ARG, "NULL ctx/in/out");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return launch(c, *in, *out, s, settled);
}

int halda_last_kernel_ms(void *ctx, double *ms) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !ms) return fail(HALDA_E_ARG, "NULL ctx/ms");
    if (!c->timed) return fail(HALDA_E_ARG, "no solve has been launched on this context");
    HIP_TRY(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms = f;
    return HALDA_OK;
}

int halda_last_solve_kernel_ms(void *ctx, double *ms) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !ms) return fail(HALDA_E_ARG, "NULL ctx/ms");
    if (!c->timed) return fail(HALDA_E_ARG, "no solve has been launched on this context");
    HIP_TRY(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, c->evs, c->ev1));
    *ms = f;
    return HALDA_OK;
}

int halda_set_timing(void *ctx, int on) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return fail(HALDA_E_ARG, "NULL ctx");
    c->timing = on != 0;
    if (!c->timing) c->timed = false;
    return HALDA_OK;
}

int halda_last_phase_ms(void *ctx, double *ms3) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !ms3) return fail(HALDA_E_ARG, "NULL ctx/ms");
    if (!c->timed) return fail(HALDA_E_ARG, "no solve has been launched on this context");
    HIP_TRY(hipEventSynchronize(c->ev1));
    float a = 0.f, b = 0.f, d = 0.f;
    if (c->fused_last) {  // no screen launch: the settled k = 1 kernel from the start
        HIP_TRY(hipEventElapsedTime(&b, c->ev0, c->evs));
    } else {
        HIP_TRY(hipEventElapsedTime(&a, c->ev0, c->evk));
        HIP_TRY(hipEventElapsedTime(&b, c->evk, c->evs));
    }
    HIP_TRY(hipEventElapsedTime(&d, c->evs, c->ev1));
    ms3[0] = a;
    ms3[1] = b;
    ms3[2] = d;
    return HALDA_OK;
}

int halda_set_fleets_path(void *ctx, int path) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return fail(HALDA_E_ARG, "NULL ctx");
    if (path < 0 || path > 6)
        return fail(HALDA_E_ARG, "path must be 0 (CSR), 1 (fused), 2 (fused, one fleet per wave), 3 (fused, k = 1 "
                                 "by DP), 4 (fused, segment kernel instead of the k-slot kernel), 5 (fused, the "
                                 "k-slot scan unsplit), 6 (fused, the k-slot split scan in sequential order)");
    c->fleets_fused = path != 0;
    c->seg_sweep = path == 1 || path == 4 || path == 5 || path == 6;
    c->kslot_sweep = path == 1 || path == 5 || path == 6;
    c->k1_force_dp = path == 3;
    c->kslot_split = path == 5 ? 0 : 2;
    c->kslot_opt = path != 6;
    ++c->path_gen;
    return HALDA_OK;
}

int halda_last_fleet_ms(void *ctx, double *ms8) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !ms8) return fail(HALDA_E_ARG, "NULL ctx/ms");
    if (!c->fleet_timed) return fail(HALDA_E_ARG, "no timed halda_solve_fleets call on this context");
    HIP_TRY(hipEventSynchronize(c->evf1));
    for (int i = 0; i < 9; ++i) ms8[i] = 0.0;
    const lrec::Slots at = lrec::record_slots(c->fleet_record);
    if (at.first >= 0) {
        float a = 0.f, b = 0.f;
        if (at.second >= 0) {
            HIP_TRY(hipEventElapsedTime(&a, c->evf0, c->evfm));
            HIP_TRY(hipEventElapsedTime(&b, c->evfm, c->evf1));
            ms8[at.first] = a;
            ms8[at.second] = b;
        } else {
            HIP_TRY(hipEventElapsedTime(&a, c->evf0, c->evf1));
            ms8[at.first] = a;  // the register launch or the table launch alone
        }
        return HALDA_OK;
    }
    if (!c->timed) return fail(HALDA_E_ARG, "no timed launch on this context");
    float lo = 0.f, a = 0.f, b = 0.f, d = 0.f, pk = 0.f;
    HIP_TRY(hipEventElapsedTime(&lo, c->evf0, c->ev0));
    HIP_TRY(hipEventElapsedTime(&a, c->ev0, c->evk));
    HIP_TRY(hipEventElapsedTime(&b, c->evk, c->evs));
    HIP_TRY(hipEventElapsedTime(&d, c->evs, c->ev1));
    HIP_TRY(hipEventElapsedTime(&pk, c->ev1, c->evf1));
    ms8[2] = lo;
    ms8[3] = a;
    ms8[4] = b;
    ms8[5] = d;
    ms8[6] = pk;
    return HALDA_OK;
}

#ifdef HALDA_STAMPS
int halda_debug_stamps(unsigned long long *out, int n_inst) {
    const int n = std::min(n_inst, kStampInst);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_halda_stamps), sizeof(unsigned long long) * kStamps * n));
    return n;
}
int halda_debug_scanprof(unsigned long long *out, int n_wave) {
    const int n = std::min(n_wave, kStampInst);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_halda_scanprof), sizeof(unsigned long long) * kScanProf * n));
    return n;
}
int halda_debug_dump(double *out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_halda_dump), sizeof(double) * kDumpFleets * kDumpDev * kDumpE * 2));
    return kDumpFleets;
}
#endif

}  // extern "C"

namespace {
// Argument checks shared by halda_solve_fleets and halda_fleets_plan_create (HALDA_OK: go on).
int check_fleets_args(const halda_model *model, const halda_fleets *fleets, const int32_t *ks, int32_t n_k,
                      const halda_fleet_result *out) {
    const halda_fleets &F = *fleets;
    if (n_k <= 0 || n_k > 1024) return fail(HALDA_E_ARG, "n_k must be in 1..1024");
    if (F.min_devices < 1 || F.max_devices < F.min_devices || F.max_devices > 4096)
        return fail(HALDA_E_ARG, "halda_fleets: need 1 <= min_devices <= max_devices <= 4096");
    if (!stage::complete(F)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    if (!out->best_k || !out->obj_value || !out->w || !out->n) return fail(HALDA_E_ARG, "halda_fleet_result: NULL");
    if (model->L < 1) return fail(HALDA_E_ARG, "model.L < 1");
    // ks (host memory): ascending, unique, positive
    for (int j = 0; j < n_k; ++j)
        if (ks[j] < 1 || (j && ks[j] <= ks[j - 1])) return fail(HALDA_E_ARG, "ks must be ascending, unique, > 0");
    return HALDA_OK;
}

// A prepared k-sweep (halda_fleets_plan_create): the fused sweep's plan, or, when the context runs
// halda_solve_fleets another way (the CSR pipeline, more than 64 k), the call's arguments.
struct FleetsPlan : CtxHandle {
    int gen = 0;  // the context's path_gen when planned
    bool fused = false;
    SweepPlan p;
    halda_model model;
    halda_fleets F;
    std::vector<int32_t> ks;
    halda_fleet_result out;
};

// (Re)derive a plan's launch sequence for its context's current path.
int replan(FleetsPlan *P) {
    Ctx *c = P->c;
    P->gen = c->path_gen;
    P->fused = P->F.n_fleets > 0 && c->fleets_fused && P->ks.size() <= 64;
    if (!P->fused) return HALDA_OK;
    return plan_sweep(c, P->model, P->F, P->ks.data(), int(P->ks.size()), P->out, &P->p);
}
}  // namespace

extern "C" {

static int fleets_csr(Ctx *c, const halda_model *model, const halda_fleets &F, const int32_t *ks, int32_t n_k,
                      halda_fleet_result *out, hipStream_t s, const halda_box *bounds);

int halda_solve_fleets(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                       int32_t n_k, halda_fleet_result *out, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !ks || !out) return fail(HALDA_E_ARG, "NULL ctx/model/fleets/ks/out");
    const halda_fleets &F = *fleets;
    if (F.n_fleets <= 0) return HALDA_OK;
    {
        const int rc = check_fleets_args(model, fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    // the fused sweep orders itself: per-stream scratch slots, and order_after_previous before a launch
    // on the context's global tables
    if (c->fleets_fused && n_k <= 64) return sweep_fleets(c, *model, F, ks, n_k, *out, s);
    return fleets_csr(c, model, F, ks, n_k, out, s, nullptr);
}

// The CSR pipeline of halda_solve_fleets (the arguments checked, the device set): the batch lowered on the
// GPU, then screened, solved and picked. bounds != nullptr (halda_solve_fleets_bounded's / _boxed's general
// route): the w columns' bounds of the lowered batch (with n bounds: the n columns' too) are overwritten
// before the solve.
static int fleets_csr(Ctx *c, const halda_model *model, const halda_fleets &F, const int32_t *ks, int32_t n_k,
                      halda_fleet_result *out, hipStream_t s, const halda_box *bounds) {
    const int32_t *kh = ks;
    {
        const int rc = order_after_previous(c, s);  // fleet_scratch / last_lowered are per context
        if (rc != HALDA_OK) return rc;
    }
    const LowerDims D = lower_dims(F.max_devices, n_k);
    const int64_t n_inst = int64_t(F.n_fleets) * n_k;
    if (n_inst > (int64_t(1) << 30) || int64_t(F.n_fleets) * D.nnz > (int64_t(1) << 31) - 1)
        return fail(HALDA_E_ARG, "batch too large for one call");
    // scratch layout
    stage::Bump lay;
    const size_t nfl = size_t(F.n_fleets);
    const size_t o_ncols = lay.take(4 * n_inst), o_nrows = lay.take(4 * n_inst), o_csr = lay.take(8 * n_inst),
                 o_col = lay.take(8 * n_inst), o_row = lay.take(8 * n_inst),
                 o_rp = lay.take(4 * nfl * size_t(D.rows + 1)), o_ci = lay.take(4 * nfl * D.nnz),
                 o_val = lay.take(8 * nfl * D.nnz), o_c = lay.take(8 * n_inst * D.cols),
                 o_clb = lay.take(8 * n_inst * D.cols), o_cub = lay.take(8 * n_inst * D.cols),
                 o_rlb = lay.take(8 * n_inst * D.rows), o_rub = lay.take(8 * n_inst * D.rows),
                 o_int = lay.take(n_inst * D.cols), o_offs = lay.take(24 * nfl), o_st = lay.take(4 * n_inst),
                 o_x = lay.take(8 * n_inst * D.cols), o_obj = lay.take(8 * n_inst), o_db = lay.take(8 * n_inst),
                 o_gap = lay.take(8 * n_inst), o_nodes = lay.take(8 * n_inst),
                 o_ks = lay.take(4 * size_t(n_k));
    {
        const int rc = grow(&c->fleet_scratch, &c->fleet_scratch_bytes, lay.off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = static_cast<char *>(c->fleet_scratch);
    // the k list travels with the stream (pageable source: the copy is staged before the call returns)
    int32_t *ks_dev = reinterpret_cast<int32_t *>(base + o_ks);
    HIP_TRY(hipMemcpyAsync(ks_dev, ks, sizeof(int32_t) * size_t(n_k), hipMemcpyHostToDevice, s));
    LowerOut O;
    O.n_cols = reinterpret_cast<int32_t *>(base + o_ncols);
    O.n_rows = reinterpret_cast<int32_t *>(base + o_nrows);
    O.csr_off = reinterpret_cast<int64_t *>(base + o_csr);
    O.col_off = reinterpret_cast<int64_t *>(base + o_col);
    O.row_off = reinterpret_cast<int64_t *>(base + o_row);
    O.row_ptr = reinterpret_cast<int32_t *>(base + o_rp);
    O.col_idx = reinterpret_cast<int32_t *>(base + o_ci);
    O.val = reinterpret_cast<double *>(base + o_val);
    O.c = reinterpret_cast<double *>(base + o_c);
    O.col_lb = reinterpret_cast<double *>(base + o_clb);
    O.col_ub = reinterpret_cast<double *>(base + o_cub);
    O.row_lb = reinterpret_cast<double *>(base + o_rlb);
    O.row_ub = reinterpret_cast<double *>(base + o_rub);
    O.integrality = reinterpret_cast<uint8_t *>(base + o_int);
    O.offs = reinterpret_cast<double *>(base + o_offs);
    c->fleet_timed = false;
    c->fleet_record = lrec::Record::csr;
    if (c->timing) HIP_TRY(hipEventRecord(c->evf0, s));
    hipLaunchKernelGGL(halda_lower_kernel, dim3(unsigned(F.n_fleets)), dim3(64), 0, s, *model, F, ks_dev, int(n_k), D,
                       O);
    HIP_TRY(hipGetLastError());
    if (bounds && (bounds->n_min || bounds->n_max)) {
        // same stream, behind the lowering: one wave per instance rewrites its M w and M n bounds
        const BoxArgs Bx{bounds->w_min, bounds->w_max, bounds->n_min, bounds->n_max};
        hipLaunchKernelGGL(halda_box_cols_kernel, dim3(unsigned((n_inst + 3) / 4)), dim3(256), 0, s, F, Bx, ks_dev,
                           int(n_k), int(model->L), int64_t(D.cols), O.col_lb, O.col_ub);
        HIP_TRY(hipGetLastError());
    } else if (bounds && (bounds->w_min || bounds->w_max)) {
        // same stream, behind the lowering: one wave per instance rewrites its M w bounds
        const BoundArgs Bd{bounds->w_min, bounds->w_max};
        hipLaunchKernelGGL(halda_bound_cols_kernel, dim3(unsigned((n_inst + 3) / 4)), dim3(256), 0, s, F, Bd, ks_dev,
                           int(n_k), int(model->L), int64_t(D.cols), O.col_lb, O.col_ub);
        HIP_TRY(hipGetLastError());
    }
    // the lowered batch and its shape summary (R = W - M with lb(w) = 1 on every device: bounds only
    // raise sum lb -- an n lower bound folded into lb(w) too -- so the slices sized here hold every bounded
    // instance too)
    halda_batch b = {};
    b.n_inst = int32_t(n_inst);
    b.max_cols = int32_t(D.cols);
    int64_t r1_k1 = 0, r1_kc = 0;
    for (int j = 0; j < n_k; ++j) {
        const int64_t r1 = int64_t(model->L / kh[j]) - F.min_devices + 1;
        if (kh[j] == 1) r1_k1 = std::max(r1_k1, r1);
        else r1_kc = std::max(r1_kc, r1);
    }
    const int64_t r1max = std::max<int64_t>(1, std::max(r1_k1, r1_kc));
    const int64_t tk1 = r1_k1 > 0 ? int64_t(F.max_devices) * r1_k1 : 0, tkc = r1_kc > 0 ? int64_t(F.max_devices) * r1_kc : 0;
    if (r1max > kMaxR1 || tk1 > (1 << 27) || tkc > (1 << 27))
        return fail(HALDA_E_ARG, "fleet shape out of range: (L / k_min - min_devices + 1) * max_devices > 2^27");
    b.max_R1 = int32_t(r1max);
    b.max_tab = int32_t(tk1);
    b.max_tab_kc = int32_t(tkc);
    b.n_cols = O.n_cols;
    b.n_rows = O.n_rows;
    b.csr_off = O.csr_off;
    b.col_off = O.col_off;
    b.row_off = O.row_off;
    b.row_ptr = O.row_ptr;
    b.col_idx = O.col_idx;
    b.val = O.val;
    b.c = O.c;
    b.col_lb = O.col_lb;
    b.col_ub = O.col_ub;
    b.row_lb = O.row_lb;
    b.row_ub = O.row_ub;
    b.integrality = O.integrality;
    b.mip_rel_gap = 0.0;
    b.mip_abs_gap = 0.0;
    b.time_limit = 0.0;
    halda_result r;
    r.status = reinterpret_cast<int32_t *>(base + o_st);
    r.x = reinterpret_cast<double *>(base + o_x);
    r.obj_lin = reinterpret_cast<double *>(base + o_obj);
    r.dual_bound = reinterpret_cast<double *>(base + o_db);
    r.gap = reinterpret_cast<double *>(base + o_gap);
    r.nodes = reinterpret_cast<int64_t *>(base + o_nodes);
    const int rc = launch(c, b, r, s);
    if (rc != HALDA_OK) return rc;
    hipLaunchKernelGGL(halda_pick_kernel, dim3(unsigned(F.n_fleets)), dim3(64), 0, s, b, r, F, int(n_k),
                       static_cast<const double *>(O.offs), *out, D.cols);
    HIP_TRY(hipGetLastError());
    if (c->timing) {
        HIP_TRY(hipEventRecord(c->evf1, s));
        c->fleet_timed = true;
    }
    c->last_lowered = b;
    c->last_solved = r;
    c->have_lowered = true;
    return HALDA_OK;
}

int halda_fleets_plan_create(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_fleet_result *out, void **plan) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !ks || !out || !plan) return fail(HALDA_E_ARG, "NULL ctx/model/fleets/ks/out/plan");
    if (fleets->n_fleets > 0) {
        const int rc = check_fleets_args(model, fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    FleetsPlan *P = new FleetsPlan();
    P->c = c;
    P->model = *model;
    P->F = *fleets;
    P->ks.assign(ks, ks + std::max(n_k, 0));
    P->out = *out;
    const int rc = replan(P);
    if (rc != HALDA_OK) {
        delete P;
        return rc;
    }
    c->handles.push_back(P);
    *plan = P;
    return HALDA_OK;
}

int halda_fleets_plan_launch(void *plan, void *stream) {
    FleetsPlan *P = static_cast<FleetsPlan *>(plan);
    if (!P) return fail(HALDA_E_ARG, "NULL plan");
    if (!P->c) return fail(HALDA_E_ARG, "halda_fleets_plan_launch: the plan's context was freed");
    if (P->F.n_fleets <= 0) return HALDA_OK;
    Ctx *c = P->c;
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    if (P->gen != c->path_gen) {  // halda_set_fleets_path since: plan the context's current path
        const int rc = replan(P);
        if (rc != HALDA_OK) return rc;
    }
    if (!P->fused)
        return halda_solve_fleets(c, &P->model, &P->F, P->ks.data(), int32_t(P->ks.size()), &P->out, stream);
    return run_sweep(c, P->p, s);
}

int halda_fleets_plan_launch_many(void *const *plans, int32_t n_plans, void *const *streams, int32_t n_streams,
                                  int64_t first, int32_t steps) {
    if (!plans || !streams || n_plans <= 0 || n_streams <= 0 || steps < 0 || first < 0)
        return fail(HALDA_E_ARG, "halda_fleets_plan_launch_many: NULL arrays or bad counts");
    for (int32_t t = 0; t < steps; ++t) {
        const int64_t i = first + t;
        const int rc = halda_fleets_plan_launch(plans[i % n_plans], streams[i % n_streams]);
        if (rc != HALDA_OK) return rc;
    }
    return HALDA_OK;
}

void halda_fleets_plan_free(void *plan) {
    FleetsPlan *P = static_cast<FleetsPlan *>(plan);
    if (!P) return;
    if (P->c) P->c->detach(P);
    delete P;
}

}  // extern "C"

// ---- groups: `steps` batches over resident tables in one launch (halda_sweep_steps_kernel)
namespace {
struct FleetsGroup : CtxHandle {
    std::vector<FleetsPlan> plans;  // copies: the group does not depend on the caller's plan handles
    bool persistent = false;        // every plan a register (or k-slot) sweep of one shape: one launch
    bool kslot = false;             // ... the k-slot form (halda_sweep_kslot_steps_kernel + gated tables)
    int gen = 0;                    // the context's path_gen when the group was checked
    SweepArgs A;                    // the first plan's arguments (shape, model, k list)
    StepsDesc *desc = nullptr;      // device copy of the plans' tables / results
    uint8_t *fflag = nullptr;       // k-slot form: per (plan, fleet) hand-back flags
    int *hb = nullptr;              // ... the launch's hand-back flag
    int64_t lds = 0;                // ... the k-slot launch's LDS (the plan's)
};

bool same_model(const halda_model &a, const halda_model &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// Whether the group's plans can run as one steps launch, and its descriptors if so.
int group_check(FleetsGroup *G) {
    Ctx *c = G->c;
    G->gen = c->path_gen;
    G->persistent = false;
    for (FleetsPlan &P : G->plans) {
        if (P.gen != c->path_gen) {
            const int rc = replan(&P);
            if (rc != HALDA_OK) return rc;
        }
    }
    const FleetsPlan &P0 = G->plans[0];
    const bool reg = P0.fused && P0.p.kind == kRegAlone && P0.p.A.uM > 0 && P0.p.A.uM <= kK1MaxM && !P0.p.A.k1dp;
    const bool ksl = P0.fused && P0.p.kind == kKslotGated;
    bool ok = (reg || ksl) && !(P0.p.A.outs & kOutXC) && !P0.p.A.x_off;
    for (const FleetsPlan &P : G->plans) {
        ok = ok && P.fused && P.p.kind == P0.p.kind && P.F.n_fleets == P0.F.n_fleets && P.p.A.uM == P0.p.A.uM &&
             P.F.min_devices == P0.F.min_devices && P.F.max_devices == P0.F.max_devices &&
             P.p.A.outs == P0.p.A.outs && P.ks == P0.ks && same_model(P.model, P0.model) && !P.p.A.x_off &&
             P.p.lds == P0.p.lds && P.p.slice == P0.p.slice && P.p.grid2 == P0.p.grid2 &&
             P.p.block1 == P0.p.block1 && std::memcmp(&P.p.SA, &P0.p.SA, sizeof(SlotArgs)) == 0;
    }
    if (!ok) return HALDA_OK;
    std::vector<StepsDesc> h(G->plans.size());
    for (size_t i = 0; i < h.size(); ++i) {
        const FleetsPlan &P = G->plans[i];
        h[i].F = P.F;
        h[i].out = FleetOut(P.out);
        int64_t base = 0;  // dev_off[0] of the table (device memory, read once here)
        HIP_TRY(hipMemcpy(&base, P.F.dev_off, sizeof base, hipMemcpyDeviceToHost));
        h[i].base = base;
        // the steps kernel indexes the table's arrays with 32-bit byte offsets (load_fields32)
        if (reg && (base < 0 || base + int64_t(P.F.n_fleets) * P0.p.A.uM > (int64_t(1) << 29))) return HALDA_OK;
    }
    if (!G->desc) HIP_TRY(hipMalloc(&G->desc, sizeof(StepsDesc) * h.size()));
    HIP_TRY(hipMemcpy(G->desc, h.data(), sizeof(StepsDesc) * h.size(), hipMemcpyHostToDevice));
    G->A = P0.p.A;
    G->kslot = ksl;
    if (ksl) {
        G->lds = P0.p.lds;
        HIP_TRY(Ctx::ensure_lds(reinterpret_cast<const void *>(halda_sweep_kslot_steps_kernel), G->lds));
        HIP_TRY(Ctx::ensure_lds(reinterpret_cast<const void *>(halda_sweep_tables_steps_kernel), P0.p.slice));
        const size_t nfl = h.size() * size_t(P0.F.n_fleets);
        if (!G->fflag) HIP_TRY(hipMalloc(&G->fflag, std::max<size_t>(nfl, 1)));
        if (!G->hb) HIP_TRY(hipMalloc(&G->hb, sizeof(int)));
        HIP_TRY(hipMemset(G->fflag, 0, std::max<size_t>(nfl, 1)));
        HIP_TRY(hipMemset(G->hb, 0, sizeof(int)));
    }
    G->persistent = true;
    return HALDA_OK;
}

// The launch of a frontier kernel (halda_solve_fleets_budget, halda_solve_change): `view` is the table under
// the count and length summary of what is solved (the fleets, or the items), `slice` the wave's LDS bytes,
// J the kernel's own arguments.
template <class Args>
int launch_frontier(Ctx *c, void (*kernel)(SweepArgs, Args), const halda_model &model,
                    const halda_fleets &view, int32_t k, int64_t slice, const Args &J, void *stream) {
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    SweepArgs A = {};
    static_cast<halda_model &>(A.Mo) = model;
    A.Mo.bvo = model_bvo(model);
    A.F = view;
    A.ks[0] = k;
    A.Ws[0] = model.L / k;
    A.n_k = 1;
    A.mmax = view.max_devices;
    A.uM = view.min_devices == view.max_devices ? view.max_devices : 0;
    A.xstride = 7 * int64_t(view.max_devices) + 1;
    int per_cu = 0;
    HIP_TRY(c->occupancy(reinterpret_cast<const void *>(kernel), slice, &per_cu));  // also raises the dynamic-LDS limit
    const unsigned grid =
        unsigned(std::max<int64_t>(1, std::min<int64_t>(int64_t(c->cus) * per_cu, int64_t(view.n_fleets))));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), size_t(slice), s, A, J);
    HIP_TRY(hipGetLastError());
    return HALDA_OK;
}
}  // namespace

extern "C" {

int halda_fleets_group_create(void *const *plans, int32_t n_plans, void **group, int32_t *persistent) {
    if (!plans || n_plans <= 0 || !group) return fail(HALDA_E_ARG, "halda_fleets_group_create: NULL arrays or n_plans <= 0");
    Ctx *c = nullptr;
    for (int32_t i = 0; i < n_plans; ++i) {
        const FleetsPlan *P = static_cast<const FleetsPlan *>(plans[i]);
        if (!P || !P->c) return fail(HALDA_E_ARG, "halda_fleets_group_create: NULL plan or freed context");
        if (c && P->c != c) return fail(HALDA_E_ARG, "halda_fleets_group_create: plans of different contexts");
        c = P->c;
    }
    HIP_TRY(hipSetDevice(c->device));
    FleetsGroup *G = new FleetsGroup();
    G->c = c;
    for (int32_t i = 0; i < n_plans; ++i) G->plans.push_back(*static_cast<const FleetsPlan *>(plans[i]));
    for (FleetsPlan &P : G->plans) P.c = c;
    const int rc = group_check(G);
    if (rc != HALDA_OK) {
        if (G->desc) (void)hipFree(G->desc);
        if (G->fflag) (void)hipFree(G->fflag);
        if (G->hb) (void)hipFree(G->hb);
        delete G;
        return rc;
    }
    c->handles.push_back(G);
    *group = G;
    if (persistent) *persistent = G->persistent ? 1 : 0;
    return HALDA_OK;
}

int halda_fleets_group_launch(void *group, int64_t first, int32_t steps, void *stream) {
    FleetsGroup *G = static_cast<FleetsGroup *>(group);
    if (!G) return fail(HALDA_E_ARG, "NULL group");
    if (!G->c) return fail(HALDA_E_ARG, "halda_fleets_group_launch: the group's context was freed");
    if (steps < 0 || first < 0) return fail(HALDA_E_ARG, "halda_fleets_group_launch: steps and first must be >= 0");
    Ctx *c = G->c;
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    if (G->gen != c->path_gen) {
        const int rc = group_check(G);
        if (rc != HALDA_OK) return rc;
    }
    const int64_t n = int64_t(G->plans.size());
    if (steps == 0 || G->plans[0].F.n_fleets <= 0) return HALDA_OK;
    if (!G->persistent) {  // batch by batch, each its own launch(es), in order on the one stream
        for (int32_t t = 0; t < steps; ++t) {
            FleetsPlan &P = G->plans[size_t((first + t) % n)];
            const int rc = P.fused ? run_sweep(c, P.p, s)
                                   : halda_solve_fleets(c, &P.model, &P.F, P.ks.data(), int32_t(P.ks.size()), &P.out, s);
            if (rc != HALDA_OK) return rc;
        }
        return HALDA_OK;
    }
    StepsArgs SG;
    SG.desc = G->desc;
    SG.n_desc = int(n);
    SG.first = int(first % n);
    SG.steps = steps;
    SG.fflag = G->fflag;
    forget_last(c);
    const int nf = G->plans[0].F.n_fleets;
    if (c->timing) HIP_TRY(hipEventRecord(c->evf0, s));
    if (G->kslot) {
        const SweepPlan &p = G->plans[0].p;
        SweepArgs A = G->A;
        stamp(c, A, nullptr, G->hb);  // (the flags per batch: SG.fflag)
        if (steps > 65535) return fail(HALDA_E_ARG, "halda_fleets_group_launch: more than 65,535 k-slot steps");
        // one workgroup per (batch, group of four fleets): the dispatcher's order is the items' order
        const unsigned ng = unsigned((nf + 64 / kSegLanes - 1) / (64 / kSegLanes));
        HIP_TRY(Ctx::ensure_lds(reinterpret_cast<const void *>(halda_sweep_kslot_steps_kernel), G->lds));
        hipLaunchKernelGGL(halda_sweep_kslot_steps_kernel, dim3(ng, unsigned(steps)), dim3(p.block1), size_t(G->lds), s,
                           A, p.SA, SG);
        HIP_TRY(hipGetLastError());
        if (c->timing) HIP_TRY(hipEventRecord(c->evfm, s));
        A.want = 1;  // the fleets flagged above, gated on the launch's hand-back flag
        HIP_TRY(Ctx::ensure_lds(reinterpret_cast<const void *>(halda_sweep_tables_steps_kernel), p.slice));
        hipLaunchKernelGGL(halda_sweep_tables_steps_kernel, dim3(p.grid2, unsigned(std::min<int64_t>(steps, n))),
                           dim3(64), size_t(p.slice), s, A, SG);
        HIP_TRY(hipGetLastError());
    } else {
        // one wave per (batch, fleet) item: grid (fleet blocks, steps)
        if (steps > 65535) return fail(HALDA_E_ARG, "halda_fleets_group_launch: more than 65,535 steps");
        hipLaunchKernelGGL(halda_sweep_steps_kernel,
                           dim3(unsigned((nf + kSweepWavesPerBlock - 1) / kSweepWavesPerBlock), unsigned(steps)),
                           dim3(64 * kSweepWavesPerBlock), 0, s, G->A, SG);
        HIP_TRY(hipGetLastError());
    }
    return finish(c, s, G->kslot ? lrec::Record::kslot_steps_then_tables : lrec::Record::steps_alone);
}

void halda_fleets_group_free(void *group) {
    FleetsGroup *G = static_cast<FleetsGroup *>(group);
    if (!G) return;
    if (G->c) {
        (void)hipSetDevice(G->c->device);
        G->c->detach(G);
    }
    if (G->desc) (void)hipFree(G->desc);
    if (G->fflag) (void)hipFree(G->fflag);
    if (G->hb) (void)hipFree(G->hb);
    delete G;
}

// Synchronous halda_solve_fleets on HOST arrays: copies the table in, solves, copies results out.
constexpr size_t kZeroCopyBytes = size_t(1) << 20;


int halda_solve_fleets_host(void *ctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks,
                            int32_t n_k, halda_fleet_result *out_h) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fh || !ks || !out_h) return fail(HALDA_E_ARG, "NULL ctx/model/fleets/ks/out");
    if (fh->n_fleets <= 0) return HALDA_OK;
    if (!fh->dev_off) return fail(HALDA_E_ARG, "halda_fleets.dev_off is NULL");
    const int64_t nf = fh->n_fleets, nd = fh->dev_off[nf];
    if (nd < nf || n_k <= 0) return fail(HALDA_E_ARG, "bad device count / n_k");
    if (!stage::complete(*fh)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // the table's fields in two blocks (10 + 6 rows): the layout's total decides the transport below
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd, 10);
    const bool xsel = stage::compact(*out_h);
    // x / c extent: the dense layout, or the caller's compact one (x_off, host memory)
    const size_t n_inst = size_t(nf) * n_k;
    const size_t xs = stage::xc_extent(fh->dev_off, nf, n_k, 1, fh->max_devices, xsel ? out_h->x_off : nullptr);
    const stage::ResultSlots R = stage::lay_result(lay, *out_h, nf, nd, n_inst, xs);
    const size_t off = lay.off;
    {
        const int rc = ensure_scratch(c, off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = static_cast<char *>(c->scratch);
    // inputs are packed into pinned host memory and cross PCIe in ONE copy (results likewise)
    if (off > c->pinned_bytes) {
        if (c->pinned) HIP_TRY(hipHostFree(c->pinned));
        c->pinned = nullptr;
        c->pinned_dev = nullptr;
        c->pinned_bytes = 0;
        // fine-grained (coherent): the resident wave reads and writes it between host accesses without a
        // kernel boundary in between
        HIP_TRY(hipHostMalloc(&c->pinned, off, hipHostMallocMapped | hipHostMallocCoherent));
        c->pinned_bytes = off;
    }
    char *pin = static_cast<char *>(c->pinned);
    const bool zc = off <= kZeroCopyBytes && !c->host_copy;
    const auto copies = stage::result_copies(R, *out_h);
    // every array in halda_host_alloc blocks (the batch API's workspaces): DMA straight from / to them
    bool direct = !zc;
    if (direct) {
        for (int a = 0; a < stage::kFields && direct; ++a) direct = in_host_block(fh->*stage::kField[a], 8 * nd);
        direct = direct && in_host_block(fh->dev_off, 8 * (nf + 1)) && in_host_block(fh->os_class, nd) &&
                 in_host_block(fh->flags, nd) && in_host_block(out_h->x_off, xsel ? 8 * n_inst : 0);
        for (const stage::Copy &k : copies) direct = direct && in_host_block(k.host, k.bytes);
    }
    auto up = [&](size_t o, const void *src, size_t bytes) {
        if (direct) return hipMemcpyAsync(static_cast<char *>(c->scratch) + o, src, bytes, hipMemcpyHostToDevice, s);
        std::memcpy(pin + o, src, bytes);
        return hipSuccess;
    };
    HIP_TRY(up(T.dev_off, fh->dev_off, 8 * (nf + 1)));
    HIP_TRY(up(T.os_class, fh->os_class, nd));
    HIP_TRY(up(T.flags, fh->flags, nd));
    for (int a = 0; a < stage::kFields; ++a) HIP_TRY(up(T.field[a], fh->*stage::kField[a], 8 * nd));
    if (xsel) HIP_TRY(up(R.x_off, out_h->x_off, 8 * n_inst));
    // small calls (a single halda_solve: ~8 KB in, ~70 KB out) skip both copies: the kernels read the
    // table from and write the results to the pinned buffer itself, across PCIe, and the host polls
    // the completion event instead of sleeping in a stream synchronisation
    if (zc) {
        if (!c->pinned_dev) HIP_TRY(hipHostGetDevicePointer(&c->pinned_dev, c->pinned, 0));
        base = static_cast<char *>(c->pinned_dev);
    } else if (!direct) {
        HIP_TRY(hipMemcpyAsync(base, pin, R.best_k, hipMemcpyHostToDevice, s));  // the table (and x_off)
    }
    const halda_fleets d = stage::rebase(*fh, base, T);
    halda_fleet_result r = stage::bind_result(base, R, *out_h, true);  // the statuses: read below (host_zero)
    // zero-copy through the fused sweep: the kernels skip the zero x / c of non-optimal instances
    // (stores across PCIe, most of a one-fleet k-sweep's time); the copy-out below zero-fills them
    const bool host_zero = zc && c->fleets_fused && (r.x || r.c) && !xsel;
    c->x_zero = !host_zero;
    bool resident = false;
    if (zc && nf == 1 && c->fleets_fused && c->resident && n_k <= 64) {
        // one fleet, the register-only plan: the resident wave, no launch
        const int rc0 = check_fleets_args(model, &d, ks, n_k, &r);
        if (rc0 != HALDA_OK) {
            c->x_zero = true;
            return rc0;
        }
        SweepPlan *p = nullptr;
        bool retry = false;
        int rc1 = cached_plan(c, *model, d, ks, n_k, r, &p);
        if (rc1 == HALDA_OK) rc1 = resident_sweep(c, *p, &resident, &retry);
        c->x_zero = rc1 != HALDA_OK || retry ? true : c->x_zero;
        if (rc1 != HALDA_OK) return rc1;
        if (retry) return halda_solve_fleets_host(ctx, model, fh, ks, n_k, out_h);  // on a fresh pinned buffer
    }
    const int rc = resident ? HALDA_OK : halda_solve_fleets(ctx, model, &d, ks, n_k, &r, s);
    c->x_zero = true;
    if (rc != HALDA_OK) return rc;
    if (resident) {
        // the results are in the pinned buffer (ack was published after them)
    } else if (zc) {
        HIP_TRY(hipEventRecord(c->ev_host, s));
        hipError_t q;
        while ((q = hipEventQuery(c->ev_host)) == hipErrorNotReady) {
        }
        HIP_TRY(q);
    } else if (direct) {
        const int rcd = download(copies, base, s);
        if (rcd != HALDA_OK) return rcd;
        HIP_TRY(hipStreamSynchronize(s));
        return HALDA_OK;
    } else {
        HIP_TRY(hipMemcpyAsync(pin + R.best_k, base + R.best_k, off - R.best_k, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    // the results are in the pinned buffer: one memcpy per array the caller passed (x / c, the last two
    // of the list, below when the host zero-fills them)
    for (size_t a = 0; a < copies.size() - (host_zero ? 2 : 0); ++a)
        if (copies[a].host) std::memcpy(copies[a].host, pin + copies[a].off, copies[a].bytes);
    if (host_zero) {
        // per (fleet, k): the kernel's x / c where the instance is optimal, zeros elsewhere
        const size_t per = xs / n_inst;
        const int32_t *st = reinterpret_cast<const int32_t *>(pin + R.status);
        for (size_t i = 0; i < n_inst; ++i) {
            const bool opt = st[i] == HALDA_STATUS_OPTIMAL;
            for (int a = 0; a < 2; ++a) {
                double *dst = a == 0 ? out_h->x : out_h->c;
                if (!dst) continue;
                if (opt) std::memcpy(dst + i * per, pin + (a == 0 ? R.x : R.c) + 8 * i * per, 8 * per);
                else std::memset(dst + i * per, 0, 8 * per);
            }
        }
    }
    return HALDA_OK;
}

// ---------------------------------------------------------------- sub-fleets of a resident table
// halda_solve_subfleets: items (parent fleet, index list) solved as the fleets of their listed devices.
// Fused route: every item of one length M' <= kK1MaxM and a batch of n_items fleets of M' devices planned
// as the register sweep alone (plan_sweep's kRegAlone: no table launch, nothing flagged -- the condition
// group_check uses) -> halda_sweep_subfleets_kernel gathers the fields per wave, no expanded table.
// Expansion route (everything else, and every call on path 1): halda_expand_subfleets_kernel writes the
// listed devices as a compact table into the context's grow-only sub_tab, whose dev_off is the items'
// sub_off, and the ordinary halda_solve_fleets runs on it into the caller's out. sub_tab is per context:
// a call that uses it runs after the previous user of the context's shared scratch on another stream
// (order_after_previous), like the global tables.
int halda_set_subfleets_path(void *ctx, int path) { return set_family_path(ctx, lrec::kSubfleets, path); }
int halda_last_subfleets_route(void *ctx, int *route) { return last_family_route(ctx, lrec::kSubfleets, route); }

// total: sub_off[n_items] when the caller knows it (the host variant), -1 to read it back where needed
static int solve_subfleets(void *ctx, const halda_model *model, const halda_fleets *table,
                           const halda_subfleets *items, const int32_t *ks, int32_t n_k, halda_fleet_result *out,
                           void *stream, int64_t total) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !table || !items || !ks || !out)
        return fail(HALDA_E_ARG, "NULL ctx/model/table/items/ks/out");
    const halda_subfleets &I = *items;
    if (I.n_items <= 0) return HALDA_OK;
    if (!I.parent || !I.sub_off || !I.sub_idx) return fail(HALDA_E_ARG, "halda_subfleets has a NULL array");
    if (table->n_fleets <= 0) return fail(HALDA_E_ARG, "halda_solve_subfleets: the table has no fleets");
    // the items seen as a batch of fleets: the table's arrays under the items' count and length summary
    halda_fleets V = *table;
    V.n_fleets = I.n_items;
    V.min_devices = I.min_devices;
    V.max_devices = I.max_devices;
    {
        const int rc = check_fleets_args(model, &V, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    const SubArgs S{I.parent, I.sub_off, I.sub_idx};
    if (c->knob[lrec::kSubfleets].path == 0 && c->fleets_fused && n_k <= 64 && I.min_devices == I.max_devices &&
        I.max_devices <= kK1MaxM) {
        SweepPlan p;
        const int rc = plan_sweep(c, *model, V, ks, n_k, *out, &p);
        if (rc != HALDA_OK) return rc;
        if (p.kind == kRegAlone && !p.A.k1dp) {
            begin_one(c, p.A);
            return launch_one(c, s, lrec::Record::reg_alone, lrec::kSubfleets, 1, [&]() -> int {
                hipLaunchKernelGGL(halda_sweep_subfleets_kernel, dim3(p.grid1), dim3(p.block1), 0, s, p.A, S);
                return launched();
            });
        }
    }
    // expansion: the listed devices as a compact table (16 double and 2 byte arrays of nd entries)
    int64_t nd = total >= 0 ? total : int64_t(I.n_items) * I.max_devices;
    if (total < 0 && I.min_devices != I.max_devices) {
        HIP_TRY(hipMemcpyAsync(&nd, I.sub_off + I.n_items, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (nd < int64_t(I.n_items) * I.min_devices || nd > int64_t(I.n_items) * I.max_devices)
            return fail(HALDA_E_ARG, "halda_subfleets: sub_off[n_items] does not fit min_devices / max_devices");
    }
    const size_t nd8 = (size_t(nd) * 8 + 255) & ~size_t(255), nd1 = (size_t(nd) + 255) & ~size_t(255);
    {
        int rc = order_after_previous(c, s);
        if (rc == HALDA_OK) rc = grow(&c->sub_tab, &c->sub_tab_bytes, 16 * nd8 + 2 * nd1);
        if (rc != HALDA_OK) return rc;
    }
    ExpandOut E;
    for (int a = 0; a < 16; ++a) E.f[a] = reinterpret_cast<double *>(c->sub_tab + nd8 * size_t(a));
    E.os_class = c->sub_tab + 16 * nd8;
    E.flags = E.os_class + nd1;
    hipLaunchKernelGGL(halda_expand_subfleets_kernel, dim3(unsigned((I.n_items + 3) / 4)), dim3(256), 0, s, *table, S,
                       int(I.n_items), E);
    HIP_TRY(hipGetLastError());
    halda_fleets X = V;
    X.dev_off = I.sub_off;
    X.os_class = E.os_class;
    X.flags = E.flags;
    for (int a = 0; a < stage::kFields; ++a) X.*stage::kField[a] = E.f[a];
    c->knob[lrec::kSubfleets].route = 2;
    return halda_solve_fleets(ctx, model, &X, ks, n_k, out, s);
}

int halda_solve_subfleets(void *ctx, const halda_model *model, const halda_fleets *table,
                          const halda_subfleets *items, const int32_t *ks, int32_t n_k, halda_fleet_result *out,
                          void *stream) {
    return solve_subfleets(ctx, model, table, items, ks, n_k, out, stream, -1);
}

// The items of a host call: sub_off from 0, parents and device indices in range, no empty list; the lists'
// shortest and longest length in *lmin / *lmax. HALDA_E_ARG with the first offender otherwise.
static int check_items_host(const halda_fleets &table, const halda_subfleets &items, int64_t *lmin_,
                            int64_t *lmax_) {
    const halda_fleets *th = &table;
    const halda_subfleets *ih = &items;
    const int64_t nf = th->n_fleets, n = ih->n_items;
    // the items: parents and device indices in range, no empty list, the length summary
    if (ih->sub_off[0] != 0) return fail(HALDA_E_ARG, "halda_subfleets: sub_off[0] must be 0");
    int64_t lmin = INT64_MAX, lmax = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p = ih->parent[i], a = ih->sub_off[i], len = ih->sub_off[i + 1] - a;
        if (p < 0 || p >= nf)
            return fail(HALDA_E_ARG, "halda_subfleets: item " + std::to_string(i) + " has parent " + std::to_string(p) +
                                         " outside the table's " + std::to_string(nf) + " fleets");
        if (len < 1) return fail(HALDA_E_ARG, "halda_subfleets: item " + std::to_string(i) + " has an empty list");
        const int64_t Mp = th->dev_off[p + 1] - th->dev_off[p];
        for (int64_t j = 0; j < len; ++j) {
            const int64_t d = ih->sub_idx[a + j];
            if (d < 0 || d >= Mp)
                return fail(HALDA_E_ARG, "halda_subfleets: item " + std::to_string(i) + " lists device " +
                                             std::to_string(d) + " of a parent with " + std::to_string(Mp) + " devices");
        }
        lmin = std::min(lmin, len);
        lmax = std::max(lmax, len);
    }
    *lmin_ = lmin;
    *lmax_ = lmax;
    return HALDA_OK;
}

int halda_solve_subfleets_host(void *ctx, const halda_model *model, const halda_fleets *th,
                               const halda_subfleets *ih, const int32_t *ks, int32_t n_k, halda_fleet_result *out_h) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !th || !ih || !ks || !out_h) return fail(HALDA_E_ARG, "NULL ctx/model/table/items/ks/out");
    if (ih->n_items <= 0) return HALDA_OK;
    if (!ih->parent || !ih->sub_off || !ih->sub_idx) return fail(HALDA_E_ARG, "halda_subfleets has a NULL array");
    if (th->n_fleets <= 0 || !th->dev_off) return fail(HALDA_E_ARG, "halda_solve_subfleets_host: empty table");
    if (n_k <= 0) return fail(HALDA_E_ARG, "n_k must be in 1..1024");
    if (!out_h->best_k || !out_h->obj_value || !out_h->w || !out_h->n)
        return fail(HALDA_E_ARG, "halda_fleet_result: NULL");
    const int64_t nf = th->n_fleets, nd = th->dev_off[nf], n = ih->n_items;
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    int64_t lmin = 0, lmax = 0;
    {
        const int rc = check_items_host(*th, *ih, &lmin, &lmax);
        if (rc != HALDA_OK) return rc;
    }
    if (lmax > 4096) return fail(HALDA_E_ARG, "halda_subfleets: a list of more than 4096 devices");
    // a summary that is given must be tight: the dense x / c layout strides by max_devices
    if ((ih->min_devices || ih->max_devices) && (lmin != ih->min_devices || lmax != ih->max_devices))
        return fail(HALDA_E_ARG, "halda_subfleets: min_devices / max_devices are not the lists' shortest and longest "
                                 "length (" + std::to_string(lmin) + ", " + std::to_string(lmax) + ")");
    const int64_t tot = ih->sub_off[n];
    if (!stage::complete(*th)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    // layout: the parent table, the item arrays, the results over the items
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const stage::ItemsLayout IL = stage::lay_items(lay, n, tot);
    const bool xsel = stage::compact(*out_h);
    const size_t xs = stage::xc_extent(ih->sub_off, n, n_k, 1, lmax, xsel ? out_h->x_off : nullptr);
    const stage::ResultSlots R = stage::lay_result(lay, *out_h, n, tot, size_t(n) * n_k, xs);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    // in: one copy per array; the call (it knows the total: no read-back); out and wait
    if (rc == HALDA_OK) rc = upload(base, T, *th, s);
    if (rc == HALDA_OK) rc = upload(base, IL, *ih, s);
    if (rc == HALDA_OK && xsel) rc = upload(base, R.x_off, out_h->x_off, 8 * R.n_inst, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*th, base, T);
    halda_subfleets di = stage::rebase(*ih, base, IL);
    di.min_devices = int32_t(lmin);
    di.max_devices = int32_t(lmax);
    halda_fleet_result r = stage::bind_result(base, R, *out_h);
    rc = solve_subfleets(ctx, model, &d, &di, ks, n_k, &r, s, tot);
    if (rc == HALDA_OK) rc = download(stage::result_copies(R, *out_h), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- exact device selection: all subsets
// halda_solve_subsets: per fleet and d = 0 .. max_drop, the best candidate (the fleet without d of its
// droppable devices) by halda_solve_subfleets' value, the earliest in enumeration order among equals.
// The host lays out one SubsetFleet per (d, fleet) and one combo list per (q, d) in use, uploads both once,
// and works d by d in launches of at most kSubsetsFusedChunk items (fused route) or kSubsetsChunkDevices
// listed devices (expansion route, cut at candidate boundaries); every launch is followed by
// halda_subsets_pick_kernel, which folds its items into the frontier. Everything lives in the context's
// grow-only sel_buf, so the call runs after the previous user of the context's shared scratch on another
// stream (order_after_previous).
constexpr int64_t kSubsetsChunkDevices = int64_t(1) << 21;
constexpr int64_t kSubsetsFusedChunk = int64_t(1) << 22;
constexpr int kSubsetsRing = 8192;  // 64-entry w / n strips of the fused route (written, never read)

int halda_set_subsets_path(void *ctx, int path) { return set_family_path(ctx, lrec::kSubsets, path); }
int halda_last_subsets_route(void *ctx, int *route) { return last_family_route(ctx, lrec::kSubsets, route); }

static int64_t binom_sat(int q, int d) {
    if (d < 0 || d > q) return 0;
    d = std::min(d, q - d);
    unsigned __int128 v = 1;
    for (int i = 1; i <= d; ++i) v = v * unsigned(q - d + i) / unsigned(i);  // exact: a product of i consecutive
    return v > (unsigned __int128)INT64_MAX ? INT64_MAX : int64_t(v);
}

int64_t halda_subsets_count(int32_t q, int32_t max_drop) {
    if (q < 0 || q > 64 || max_drop < 0) return -1;
    int64_t tot = 0;
    for (int d = 0; d <= std::min(max_drop, q); ++d) {
        const int64_t b = binom_sat(q, d);
        if (b > INT64_MAX - tot) return INT64_MAX;
        tot += b;
    }
    return tot;
}

// The combos of d of q slots in enumeration order: ascending index lists, lexicographic.
static void subset_combos(int q, int d, std::vector<uint64_t> &out) {
    int idx[64];
    for (int j = 0; j < d; ++j) idx[j] = j;
    while (true) {
        uint64_t m = 0;
        for (int j = 0; j < d; ++j) m |= uint64_t(1) << idx[j];
        out.push_back(m);
        int j = d - 1;
        while (j >= 0 && idx[j] == q - d + j) --j;
        if (j < 0) return;
        ++idx[j];
        for (int t = j + 1; t < d; ++t) idx[t] = idx[t - 1] + 1;
    }
}

struct SubsetLaunch {
    int d;
    bool fused;
    int64_t i0, n, l0, nd;  // first item, items, listed devices in front of it, its listed devices
    int lmin, lmax;         // expansion: the shortest and longest list of the launch
};

// sizes: every fleet's device count (host); keep: host masks or NULL
static int solve_subsets(void *ctx, const halda_model *model, const halda_fleets *table, const int32_t *sizes,
                         const halda_subsets *subsets, const int32_t *ks, int32_t n_k,
                         halda_subset_frontier *frontier, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    const int nf = table->n_fleets, D = subsets->max_drop;
    const uint64_t *keep = subsets->keep_mask;
    if (!frontier->status || !frontier->obj || !frontier->dropped_mask || !frontier->best_k)
        return fail(HALDA_E_ARG, "halda_subset_frontier: NULL");
    if (D < 0 || D > 63) return fail(HALDA_E_ARG, "halda_subsets: max_drop must be in 0..63");
    if (n_k <= 0 || n_k > 1024) return fail(HALDA_E_ARG, "n_k must be in 1..1024");
    if (model->L < 1) return fail(HALDA_E_ARG, "model.L < 1");
    for (int j = 0; j < n_k; ++j)
        if (ks[j] < 1 || (j && ks[j] <= ks[j - 1])) return fail(HALDA_E_ARG, "ks must be ascending, unique, > 0");
    if (!stage::complete(*table)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    // the gate, from the shapes alone
    std::vector<uint64_t> drop(nf);
    std::vector<int> qs(nf), Df(nf);
    int Dmax = -1;
    bool uniform = true;
    for (int f = 0; f < nf; ++f) {
        const int M = sizes[f];
        if (M < 1 || M > 64)
            return fail(HALDA_E_ARG, "halda_solve_subsets: fleet " + std::to_string(f) + " has " + std::to_string(M) +
                                         " devices (1..64)");
        const uint64_t all = M == 64 ? ~uint64_t(0) : (uint64_t(1) << M) - 1, k = keep ? keep[f] : 0;
        if (k & ~all)
            return fail(HALDA_E_ARG, "halda_subsets: keep_mask of fleet " + std::to_string(f) + " names a device past " +
                                         std::to_string(M));
        drop[f] = all & ~k;
        qs[f] = __builtin_popcountll(drop[f]);
        Df[f] = std::min({D, qs[f], M - 1});
        Dmax = std::max(Dmax, Df[f]);
        uniform = uniform && M == sizes[0];
        const int64_t cnt = halda_subsets_count(qs[f], Df[f]);
        if (cnt > HALDA_SUBSETS_MAX)
            return fail(HALDA_E_ARG, "halda_solve_subsets: fleet " + std::to_string(f) + " has " + std::to_string(cnt) +
                                         " candidates, the limit is " + std::to_string(HALDA_SUBSETS_MAX));
    }
    if (D > Dmax)
        return fail(HALDA_E_ARG, "halda_subsets: max_drop " + std::to_string(D) + " is beyond min(q, M - 1) = " +
                                     std::to_string(Dmax) + " of every fleet");
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    // the combo lists of every (q, d) in use, and the records per (d, fleet)
    std::vector<uint64_t> combos;
    std::vector<int64_t> coff(65 * 64, -1);
    std::vector<SubsetFleet> recs(size_t(D + 1) * nf);
    std::vector<SubsetLaunch> launches;
    int64_t max_items = 0, max_dev = 0;
    bool any_fused = false, any_expand = false;
    for (int d = 0; d <= D; ++d) {
        SubsetFleet *R = recs.data() + size_t(d) * nf;
        int64_t cmax = 0;
        for (int f = 0; f < nf; ++f) {
            SubsetFleet &r = R[f];
            r = SubsetFleet{};
            r.drop_mask = drop[f];
            r.M = sizes[f];
            r.cnt = d <= Df[f] ? int32_t(binom_sat(qs[f], d)) : 0;
            if (r.cnt > 0) {
                int64_t &o = coff[size_t(qs[f]) * 64 + d];
                if (o < 0) {
                    o = int64_t(combos.size());
                    subset_combos(qs[f], d, combos);
                }
                r.combo_off = o;
            }
            cmax = std::max<int64_t>(cmax, r.cnt);
        }
        // the route of this d: the sub-fleet kernel's gate on a batch of the d's items
        bool fused = false;
        SweepPlan p;
        const int64_t padded = cmax * nf;
        if (c->knob[lrec::kSubsets].path == 0 && c->fleets_fused && n_k <= 64 && uniform && padded < (int64_t(1) << 31)) {
            halda_fleets V = *table;
            V.n_fleets = int32_t(std::min(padded, kSubsetsFusedChunk));
            V.min_devices = V.max_devices = sizes[0] - d;
            halda_fleet_result o = {};
            const int rc = plan_sweep(c, *model, V, ks, n_k, o, &p);
            if (rc != HALDA_OK) return rc;
            fused = p.kind == kRegAlone && !p.A.k1dp;
        }
        if (fused) {
            for (int f = 0; f < nf; ++f) R[f].item_off = int64_t(f) * cmax;
            for (int64_t a = 0; a < padded; a += kSubsetsFusedChunk)
                launches.push_back(SubsetLaunch{d, true, a, std::min(kSubsetsFusedChunk, padded - a), cmax, 0, 0, 0});
            max_items = std::max(max_items, std::min(kSubsetsFusedChunk, padded));
            any_fused = true;
        } else {
            int64_t items = 0, devs = 0;
            for (int f = 0; f < nf; ++f) {
                R[f].item_off = items;
                R[f].list_off = devs;
                items += R[f].cnt;
                devs += int64_t(R[f].cnt) * (sizes[f] - d);
            }
            // chunks of at most kSubsetsChunkDevices listed devices, cut at candidate boundaries
            int f = 0;
            int64_t a = 0;
            while (a < items) {
                SubsetLaunch L{d, false, a, 0, 0, 0, 64, 0};
                while (R[f].cnt == 0 || R[f].item_off + R[f].cnt <= a) ++f;
                L.l0 = R[f].list_off + (a - R[f].item_off) * (sizes[f] - d);
                int64_t b = a;
                for (int g = f; g < nf && b < items; ++g) {
                    if (R[g].cnt == 0) continue;
                    const int len = sizes[g] - d;
                    const int64_t left = R[g].item_off + R[g].cnt - b;
                    int64_t take = std::min<int64_t>(left, (kSubsetsChunkDevices - L.nd) / len);
                    if (take <= 0) break;
                    take = std::min<int64_t>(take, INT32_MAX / 2 - L.n);
                    L.n += take;
                    L.nd += take * len;
                    L.lmin = std::min(L.lmin, len);
                    L.lmax = std::max(L.lmax, len);
                    b += take;
                    if (take < left) break;
                }
                launches.push_back(L);
                max_items = std::max(max_items, L.n);
                max_dev = std::max(max_dev, L.nd);
                a = b;
            }
            any_expand = true;
        }
        // (fused launches carry cmax in l0: the expansion fields are unused there)
    }
    // scratch: combos, records, per-item results, then the fused ring or the expansion's item arrays and w / n
    stage::Bump lay;
    const size_t o_combo = lay.take(8 * combos.size()), o_rec = lay.take(sizeof(SubsetFleet) * recs.size()),
                 o_obj = lay.take(8 * size_t(max_items)), o_bk = lay.take(4 * size_t(max_items)),
                 o_par = lay.take(4 * size_t(max_items)), o_soff = lay.take(8 * size_t(max_items + 1));
    const size_t wn = std::max<size_t>(size_t(max_dev), any_fused ? size_t(kSubsetsRing) * 64 : 0);
    const size_t o_sidx = lay.take(4 * size_t(max_dev)), o_w = lay.take(4 * wn), o_n = lay.take(4 * wn);
    {
        int rc = order_after_previous(c, s);
        if (rc == HALDA_OK) rc = grow(&c->sel_buf, &c->sel_bytes, lay.off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = reinterpret_cast<char *>(c->sel_buf);
    // (pageable sources: the copies are staged before the calls return)
    HIP_TRY(hipMemcpyAsync(base + o_combo, combos.data(), 8 * combos.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + o_rec, recs.data(), sizeof(SubsetFleet) * recs.size(), hipMemcpyHostToDevice, s));
    halda_fleet_result out = {};
    out.best_k = reinterpret_cast<int32_t *>(base + o_bk);
    out.obj_value = reinterpret_cast<double *>(base + o_obj);
    out.w = reinterpret_cast<int32_t *>(base + o_w);
    out.n = reinterpret_cast<int32_t *>(base + o_n);
    const SubsetFrontier FR{frontier->status, frontier->obj, frontier->dropped_mask, frontier->best_k};
    c->fleet_timed = false;
    for (const SubsetLaunch &L : launches) {
        SubsetArgs U = {};
        U.fl = reinterpret_cast<const SubsetFleet *>(base + o_rec) + size_t(L.d) * nf;
        U.combos = reinterpret_cast<const uint64_t *>(base + o_combo);
        U.i0 = L.i0;
        U.n = int32_t(L.n);
        U.n_fleets = nf;
        U.d = L.d;
        if (L.fused) {
            U.cmax = int32_t(L.l0);
            halda_fleets V = *table;
            V.n_fleets = int32_t(L.n);
            V.min_devices = V.max_devices = sizes[0] - L.d;
            SweepPlan p;
            const int rc = plan_sweep(c, *model, V, ks, n_k, out, &p);
            if (rc != HALDA_OK) return rc;
            // (no events, no record, and fleet_timed as an expansion launch of this call may have left it)
            stamp(c, p.A, nullptr, c->hb_flag);
            c->have_lowered = false;
            hipLaunchKernelGGL(halda_sweep_subsets_kernel,
                               dim3(unsigned((L.n + kSweepWavesPerBlock - 1) / kSweepWavesPerBlock)),
                               dim3(64 * kSweepWavesPerBlock), 0, s, p.A, U, kSubsetsRing - 1);
            HIP_TRY(hipGetLastError());
        } else {
            U.l0 = L.l0;
            halda_subfleets I;
            I.n_items = int32_t(L.n);
            I.min_devices = L.lmin;
            I.max_devices = L.lmax;
            I.parent = reinterpret_cast<const int32_t *>(base + o_par);
            I.sub_off = reinterpret_cast<const int64_t *>(base + o_soff);
            I.sub_idx = reinterpret_cast<const int32_t *>(base + o_sidx);
            hipLaunchKernelGGL(halda_subsets_index_kernel, dim3(unsigned((L.n + 3) / 4)), dim3(256), 0, s, U,
                               reinterpret_cast<int32_t *>(base + o_par), reinterpret_cast<int64_t *>(base + o_soff),
                               reinterpret_cast<int32_t *>(base + o_sidx));
            HIP_TRY(hipGetLastError());
            // the sub-fleet entry's expansion route, unedited, on the items just written
            const lrec::PathOverride expand(c->knob[lrec::kSubfleets], 1, /*keep_route=*/true);
            const int rc = solve_subfleets(ctx, model, table, &I, ks, n_k, &out, s, L.nd);
            if (rc != HALDA_OK) return rc;
        }
        hipLaunchKernelGGL(halda_subsets_pick_kernel, dim3(unsigned(nf)), dim3(256), 0, s, U,
                           static_cast<const double *>(out.obj_value), static_cast<const int32_t *>(out.best_k), FR,
                           D + 1);
        HIP_TRY(hipGetLastError());
    }
    c->knob[lrec::kSubsets].route = any_fused && any_expand ? 3 : any_fused ? 1 : 2;
    return HALDA_OK;
}

int halda_solve_subsets(void *ctx, const halda_model *model, const halda_fleets *fleets, const halda_subsets *subsets,
                        const int32_t *ks, int32_t n_k, halda_subset_frontier *frontier, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !subsets || !ks || !frontier)
        return fail(HALDA_E_ARG, "NULL ctx/model/fleets/subsets/ks/frontier");
    const int64_t nf = fleets->n_fleets;
    if (nf <= 0) return HALDA_OK;
    if (!fleets->dev_off) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    std::vector<int32_t> sizes(size_t(nf), fleets->max_devices);
    if (fleets->min_devices != fleets->max_devices) {
        HIP_TRY(hipSetDevice(c->device));
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
        std::vector<int64_t> off(size_t(nf) + 1);
        HIP_TRY(hipMemcpyAsync(off.data(), fleets->dev_off, 8 * (nf + 1), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int64_t f = 0; f < nf; ++f)
            sizes[f] = int32_t(std::max<int64_t>(-1, std::min<int64_t>(off[f + 1] - off[f], 65)));
    }
    return solve_subsets(ctx, model, fleets, sizes.data(), subsets, ks, n_k, frontier, stream);
}

int halda_solve_subsets_host(void *ctx, const halda_model *model, const halda_fleets *th, const halda_subsets *subsets,
                             const int32_t *ks, int32_t n_k, halda_subset_frontier *fh) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !th || !subsets || !ks || !fh)
        return fail(HALDA_E_ARG, "NULL ctx/model/fleets/subsets/ks/frontier");
    if (th->n_fleets <= 0) return HALDA_OK;
    if (!stage::complete(*th)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    if (!fh->status || !fh->obj || !fh->dropped_mask || !fh->best_k)
        return fail(HALDA_E_ARG, "halda_subset_frontier: NULL");
    if (subsets->max_drop < 0 || subsets->max_drop > 63)
        return fail(HALDA_E_ARG, "halda_subsets: max_drop must be in 0..63");
    const int64_t nf = th->n_fleets, nd = th->dev_off[nf];
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    std::vector<int32_t> sizes(size_t(nf), 0);
    for (int64_t f = 0; f < nf; ++f)
        sizes[f] = int32_t(std::max<int64_t>(-1, std::min<int64_t>(th->dev_off[f + 1] - th->dev_off[f], 65)));
    const size_t pts = size_t(nf) * size_t(subsets->max_drop + 1);
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const size_t o_st = lay.take(4 * pts), o_obj = lay.take(8 * pts), o_mask = lay.take(8 * pts), o_bk = lay.take(4 * pts);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *th, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*th, base, T);
    halda_subset_frontier fd;
    fd.status = reinterpret_cast<int32_t *>(base + o_st);
    fd.obj = reinterpret_cast<double *>(base + o_obj);
    fd.dropped_mask = reinterpret_cast<uint64_t *>(base + o_mask);
    fd.best_k = reinterpret_cast<int32_t *>(base + o_bk);
    rc = solve_subsets(ctx, model, &d, sizes.data(), subsets, ks, n_k, &fd, s);
    if (rc != HALDA_OK) return rc;
    const std::array<stage::Copy, 4> back = {{{fh->status, o_st, 4 * pts},
                                              {fh->obj, o_obj, 8 * pts},
                                              {fh->dropped_mask, o_mask, 8 * pts},
                                              {fh->best_k, o_bk, 4 * pts}}};
    rc = download(back, base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- model variants of one table
// halda_solve_variants: one fleet table solved for n_var models (the same L, has_f_q and has_f_out: what
// the packed table and the plan's shapes depend on), outputs variant-major, slice v bit for bit what
// halda_solve_fleets(&models[v]) writes.
// Loop route (the specification; every call on path 1): n_var calls of halda_solve_fleets on the caller's
// stream, the output pointers moved to the variant's slice.
// Fused route: one launch, blockIdx.y the variant, for the two plans in which one wave owns one fleet from
// start to end -- kRegAlone with one fleet size <= kK1MaxM (halda_sweep_variants_kernel) and kTablesAlone
// (halda_sweep_tables_variants_kernel). The plan is that of one variant (plan_sweep reads only L of the
// model, and compares the fleet count alone with kSweepSmallBatch). The variants' models go into the
// context's grow-only var_desc with the stream; var_desc is per context, so the call runs after the
// previous user of the context's shared scratch on another stream (order_after_previous).
int halda_set_variants_path(void *ctx, int path) { return set_family_path(ctx, lrec::kVariants, path); }
int halda_last_variants_route(void *ctx, int *route) { return last_family_route(ctx, lrec::kVariants, route); }

static int check_variants(const halda_model *models, int32_t n_var) {
    if (n_var < 1 || n_var > 65535) return fail(HALDA_E_ARG, "n_var must be in 1..65535");
    for (int32_t v = 1; v < n_var; ++v) {
        if (models[v].L != models[0].L)
            return fail(HALDA_E_ARG, "halda_solve_variants: variant " + std::to_string(v) + " has L = " +
                                         std::to_string(models[v].L) + ", variant 0 has L = " +
                                         std::to_string(models[0].L));
        if (!models[v].has_f_q != !models[0].has_f_q || !models[v].has_f_out != !models[0].has_f_out)
            return fail(HALDA_E_ARG, "halda_solve_variants: variant " + std::to_string(v) +
                                         " differs from variant 0 in has_f_q / has_f_out");
    }
    return HALDA_OK;
}

// total: dev_off[n_fleets] when the caller knows it (the host variant), -1 to read it back where needed
static int solve_variants(void *ctx, const halda_model *models, int32_t n_var, const halda_fleets *fleets,
                          const int32_t *ks, int32_t n_k, halda_fleet_result *out, void *stream, int64_t total) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !models || !fleets || !ks || !out) return fail(HALDA_E_ARG, "NULL ctx/models/fleets/ks/out");
    {
        const int rc = check_variants(models, n_var);
        if (rc != HALDA_OK) return rc;
    }
    const halda_fleets &F = *fleets;
    if (F.n_fleets <= 0) return HALDA_OK;
    for (int32_t v = 0; v < n_var; ++v) {
        const int rc = check_fleets_args(&models[v], fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    const int64_t nf = F.n_fleets;
    // the fused kernels index fleets and (fleet, k) instances over all variants with 32 bits
    if (c->knob[lrec::kVariants].path == 0 && c->fleets_fused && n_k <= 64 && int64_t(n_var) * nf * n_k < (int64_t(1) << 31)) {
        SweepPlan p;
        const int rc = plan_sweep(c, models[0], F, ks, n_k, *out, &p);
        if (rc != HALDA_OK) return rc;
        const bool reg = p.kind == kRegAlone && p.A.uM > 0 && p.A.uM <= kK1MaxM && !p.A.k1dp;
        if (reg || p.kind == kTablesAlone) {
            std::vector<SweepModel> h{size_t(n_var), SweepModel{}};
            for (int32_t v = 0; v < n_var; ++v) {
                static_cast<halda_model &>(h[v]) = models[v];
                h[v].bvo = model_bvo(models[v]);
            }
            {
                int rc2 = order_after_previous(c, s);
                if (rc2 == HALDA_OK) rc2 = grow(&c->var_desc, &c->var_desc_bytes, sizeof(SweepModel) * h.size());
                if (rc2 != HALDA_OK) return rc2;
            }
            // (pageable source: the copy is staged before the call returns)
            HIP_TRY(hipMemcpyAsync(c->var_desc, h.data(), sizeof(SweepModel) * h.size(), hipMemcpyHostToDevice, s));
            const VarArgs V{reinterpret_cast<const SweepModel *>(c->var_desc)};
            SweepArgs &A = p.A;
            begin_one(c, A);  // neither plan flags: one launch, nothing behind it
            if (reg)
                return launch_one(c, s, lrec::Record::reg_alone, lrec::kVariants, 1, [&]() -> int {
                    hipLaunchKernelGGL(halda_sweep_variants_kernel, dim3(p.grid1, unsigned(n_var)), dim3(p.block1), 0,
                                       s, A, V);
                    return launched();
                });
            A.uM = 0;  // every extent from dev_off (the kernel moves its view of it per variant)
            const void *fn = reinterpret_cast<const void *>(halda_sweep_tables_variants_kernel);
            HIP_TRY(Ctx::ensure_lds(fn, p.lds));
            return launch_one(c, s, lrec::Record::tables_alone, lrec::kVariants, 1, [&]() -> int {
                hipLaunchKernelGGL(halda_sweep_tables_variants_kernel, dim3(p.grid1, unsigned(n_var)), dim3(64),
                                   size_t(p.lds), s, A, V);
                return launched();
            });
        }
    }
    // the loop: variant v's slice of every output
    int64_t nd = total;
    if (nd < 0 && n_var > 1) {
        HIP_TRY(hipMemcpyAsync(&nd, F.dev_off + nf, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (nd < 0) return fail(HALDA_E_ARG, "halda_fleets: dev_off[n_fleets] < 0");
    }
    const int64_t xstride = 7 * int64_t(std::max(F.max_devices, 1)) + 1;
    c->knob[lrec::kVariants].route = 2;
    for (int64_t v = 0; v < n_var; ++v) {
        // (nd is not read back for one variant: slice 0 asks for no offset)
        halda_fleet_result o = lrec::result_slice(*out, v, nf, v ? v * nd : 0, n_k, xstride);
        const int rc = halda_solve_fleets(ctx, &models[v], fleets, ks, n_k, &o, s);
        if (rc != HALDA_OK) return rc;
    }
    return HALDA_OK;
}

int halda_solve_variants(void *ctx, const halda_model *models, int32_t n_var, const halda_fleets *fleets,
                         const int32_t *ks, int32_t n_k, halda_fleet_result *out, void *stream) {
    return solve_variants(ctx, models, n_var, fleets, ks, n_k, out, stream, -1);
}

int halda_solve_variants_host(void *ctx, const halda_model *models, int32_t n_var, const halda_fleets *fh,
                              const int32_t *ks, int32_t n_k, halda_fleet_result *out_h) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !models || !fh || !ks || !out_h) return fail(HALDA_E_ARG, "NULL ctx/models/fleets/ks/out");
    {
        const int rc = check_variants(models, n_var);
        if (rc != HALDA_OK) return rc;
    }
    if (fh->n_fleets <= 0) return HALDA_OK;
    if (!fh->dev_off) return fail(HALDA_E_ARG, "halda_fleets.dev_off is NULL");
    if (n_k <= 0 || n_k > 1024) return fail(HALDA_E_ARG, "n_k must be in 1..1024");
    if (!out_h->best_k || !out_h->obj_value || !out_h->w || !out_h->n)
        return fail(HALDA_E_ARG, "halda_fleet_result: NULL");
    const int64_t nf = fh->n_fleets, nd = fh->dev_off[nf], nv = n_var;
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    if (!stage::complete(*fh)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    // layout: the table, once; the results variant-major over (variant, fleet, k)
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const bool xsel = stage::compact(*out_h);
    const size_t xs = stage::xc_extent(fh->dev_off, nf, n_k, nv, fh->max_devices, xsel ? out_h->x_off : nullptr);
    const stage::ResultSlots R = stage::lay_result(lay, *out_h, nv * nf, nv * nd, size_t(nv) * nf * n_k, xs);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    // in: one copy per array; the call (it knows the total: no read-back); out, only the variants' slices
    if (rc == HALDA_OK) rc = upload(base, T, *fh, s);
    if (rc == HALDA_OK && xsel) rc = upload(base, R.x_off, out_h->x_off, 8 * R.n_inst, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*fh, base, T);
    halda_fleet_result r = stage::bind_result(base, R, *out_h);
    rc = solve_variants(ctx, models, n_var, &d, ks, n_k, &r, s, nd);
    if (rc == HALDA_OK) rc = download(stage::result_copies(R, *out_h), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- a caller's plan priced on the table
// halda_eval_plans: fleet f's plan (k, w, n) evaluated on the table (halda_eval_plans_kernel, any shape).
// halda_solve_fleets_plans: the k-sweep of the table plus the evaluation of the incumbent plans.
// Two-launch route (the default, every shape): halda_eval_plans_kernel, then halda_solve_fleets, both on the
// caller's stream. Fused route (path 2): where the sweep is the register launch alone over fleets of one size
// <= kK1MaxM (kRegAlone, the sub-fleet and variants kernels' gate), ONE launch of halda_sweep_plans_kernel --
// each wave prices its fleet's plan on the fields it loads for the sweep.
int halda_set_plans_path(void *ctx, int path) { return set_family_path(ctx, lrec::kPlans, path); }
int halda_last_plans_route(void *ctx, int *route) { return last_family_route(ctx, lrec::kPlans, route); }

// Argument checks of the plan entries, before any HIP call (HALDA_OK: go on).
static int check_plans_args(const void *ctx, const halda_model *model, const halda_fleets *fleets,
                            const halda_plans *plans, const halda_plan_result *out, const char *who) {
    if (!ctx || !model || !fleets || !plans || !out)
        return fail(HALDA_E_ARG, std::string(who) + ": NULL ctx/model/fleets/plans/out");
    if (fleets->n_fleets < 0) return fail(HALDA_E_ARG, std::string(who) + ": n_fleets < 0");
    if (!plans->k || !plans->w || !plans->n) return fail(HALDA_E_ARG, std::string(who) + ": halda_plans has a NULL array");
    if (!out->status || !out->obj_value)
        return fail(HALDA_E_ARG, std::string(who) + ": halda_plan_result needs status and obj_value");
    if (model->L < 1) return fail(HALDA_E_ARG, "model.L < 1");
    return HALDA_OK;
}

static int check_plans_table(const halda_fleets &F) {
    if (F.min_devices < 1 || F.max_devices < F.min_devices || F.max_devices > 4096)
        return fail(HALDA_E_ARG, "halda_fleets: need 1 <= min_devices <= max_devices <= 4096");
    if (!stage::complete(F)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    return HALDA_OK;
}

static PlanArgs plan_args(const halda_fleets &F, const halda_plans &P, const halda_plan_result &O) {
    PlanArgs E = {};
    E.k = P.k; E.w = P.w; E.n = P.n;
    E.status = O.status; E.obj_value = O.obj_value; E.cycle = O.cycle; E.bottleneck = O.bottleneck;
    E.reason = O.reason; E.x = O.x; E.c = O.c; E.x_off = O.x_off;
    E.xstride = 7 * int64_t(std::max(F.max_devices, 1)) + 1;
    E.outs = (O.x ? kOutX : 0) | (O.c ? kOutC : 0) | (O.cycle ? kPlanOutCycle : 0) |
             (O.bottleneck ? kPlanOutBott : 0) | (O.reason ? kPlanOutReason : 0);
    return E;
}

static int launch_eval_plans(const halda_model &model, const halda_fleets &F, const PlanArgs &E, hipStream_t s) {
    EvalArgs A;
    static_cast<halda_model &>(A.Mo) = model;
    A.Mo.bvo = model_bvo(model);
    A.F = F;
    A.E = E;
    hipLaunchKernelGGL(halda_eval_plans_kernel, dim3(unsigned((int64_t(F.n_fleets) + 3) / 4)), dim3(256), 0, s, A);
    HIP_TRY(hipGetLastError());
    return HALDA_OK;
}

int halda_eval_plans(void *ctx, const halda_model *model, const halda_fleets *fleets, const halda_plans *plans,
                     halda_plan_result *out, void *stream) {
    {
        const int rc = check_plans_args(ctx, model, fleets, plans, out, "halda_eval_plans");
        if (rc != HALDA_OK) return rc;
    }
    Ctx *c = static_cast<Ctx *>(ctx);
    const halda_fleets &F = *fleets;
    if (F.n_fleets == 0) return HALDA_OK;
    {
        const int rc = check_plans_table(F);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    return launch_eval_plans(*model, F, plan_args(F, *plans, *out), s);
}

int halda_solve_fleets_plans(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_plans *plans, halda_plan_result *eval_out,
                             halda_fleet_result *out, void *stream) {
    {
        const int rc = check_plans_args(ctx, model, fleets, plans, eval_out, "halda_solve_fleets_plans");
        if (rc != HALDA_OK) return rc;
    }
    if (!ks || !out) return fail(HALDA_E_ARG, "halda_solve_fleets_plans: NULL ks/out");
    Ctx *c = static_cast<Ctx *>(ctx);
    const halda_fleets &F = *fleets;
    if (F.n_fleets == 0) return HALDA_OK;
    {
        const int rc = check_fleets_args(model, fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    const PlanArgs E = plan_args(F, *plans, *eval_out);
    // automatic = two launches: the fused launch measured 7 % ahead of them on C3's shape, inside the
    // box-to-box spread, so it stays behind path 2
    if (c->knob[lrec::kPlans].path == 2 && c->fleets_fused && n_k <= 64) {
        SweepPlan p;
        const int rc = plan_sweep(c, *model, F, ks, n_k, *out, &p);
        if (rc != HALDA_OK) return rc;
        if (p.kind == kRegAlone && p.A.uM > 0 && p.A.uM <= kK1MaxM && !p.A.k1dp) {
            begin_one(c, p.A);
            return launch_one(c, s, lrec::Record::reg_alone, lrec::kPlans, 1, [&]() -> int {
                hipLaunchKernelGGL(halda_sweep_plans_kernel, dim3(p.grid1), dim3(p.block1), 0, s, p.A, E);
                return launched();
            });
        }
    }
    {
        const int rc = launch_eval_plans(*model, F, E, s);
        if (rc != HALDA_OK) return rc;
    }
    c->knob[lrec::kPlans].route = 2;
    return halda_solve_fleets(ctx, model, fleets, ks, n_k, out, s);
}

// The host variants: the table, the plans (and x_off) cross PCIe once on the way in, the results on the way
// out, through the context's staging scratch. out_h == nullptr: the evaluation alone.
static int plans_host(void *ctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks, int32_t n_k,
                      const halda_plans *ph, halda_plan_result *eh, halda_fleet_result *out_h) {
    Ctx *c = static_cast<Ctx *>(ctx);
    const int64_t nf = fh->n_fleets;
    if (nf == 0) return HALDA_OK;
    if (!fh->dev_off) return fail(HALDA_E_ARG, "halda_fleets.dev_off is NULL");
    {
        const int rc = check_plans_table(*fh);
        if (rc != HALDA_OK) return rc;
    }
    if (out_h) {
        if (n_k <= 0 || n_k > 1024) return fail(HALDA_E_ARG, "n_k must be in 1..1024");
        if (!out_h->best_k || !out_h->obj_value || !out_h->w || !out_h->n)
            return fail(HALDA_E_ARG, "halda_fleet_result: NULL");
    }
    const int64_t nd = fh->dev_off[nf];
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    // layout: the table; the plans and the evaluation's outputs; the sweep's outputs (none: the same slots, empty)
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const size_t o_pk = lay.take(4 * nf), o_pw = lay.take(4 * nd), o_pn = lay.take(4 * nd);
    const size_t o_est = lay.take(4 * nf), o_eobj = lay.take(8 * nf), o_ecyc = lay.take(8 * nf),
                 o_ebot = lay.take(4 * nf), o_erea = lay.take(4 * nf);
    const bool exsel = eh->x_off && (eh->x || eh->c);
    const size_t o_exoff = exsel ? lay.take(8 * nf) : 0;
    const size_t exs = stage::xc_extent(fh->dev_off, nf, 1, 1, fh->max_devices, exsel ? eh->x_off : nullptr);
    const size_t o_ex = eh->x ? lay.take(8 * exs) : 0, o_ec = eh->c ? lay.take(8 * exs) : 0;
    const halda_fleet_result none = {};
    const halda_fleet_result &oh = out_h ? *out_h : none;
    const bool xsel = stage::compact(oh);
    const int64_t nk = out_h ? n_k : 0;
    const size_t xs = stage::xc_extent(fh->dev_off, nf, nk, 1, fh->max_devices, xsel ? oh.x_off : nullptr);
    const stage::ResultSlots R = stage::lay_result(lay, oh, nf, nd, size_t(nf) * nk, xs);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *fh, s);
    if (rc == HALDA_OK) rc = upload(base, o_pk, ph->k, 4 * nf, s);
    if (rc == HALDA_OK) rc = upload(base, o_pw, ph->w, 4 * nd, s);
    if (rc == HALDA_OK) rc = upload(base, o_pn, ph->n, 4 * nd, s);
    if (rc == HALDA_OK && exsel) rc = upload(base, o_exoff, eh->x_off, 8 * nf, s);
    if (rc == HALDA_OK && xsel) rc = upload(base, R.x_off, oh.x_off, 8 * R.n_inst, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*fh, base, T);
    halda_plans dp;
    dp.k = reinterpret_cast<const int32_t *>(base + o_pk);
    dp.w = reinterpret_cast<const int32_t *>(base + o_pw);
    dp.n = reinterpret_cast<const int32_t *>(base + o_pn);
    halda_plan_result de;
    de.status = reinterpret_cast<int32_t *>(base + o_est);
    de.obj_value = reinterpret_cast<double *>(base + o_eobj);
    de.cycle = eh->cycle ? reinterpret_cast<double *>(base + o_ecyc) : nullptr;
    de.bottleneck = eh->bottleneck ? reinterpret_cast<int32_t *>(base + o_ebot) : nullptr;
    de.reason = eh->reason ? reinterpret_cast<int32_t *>(base + o_erea) : nullptr;
    de.x = eh->x ? reinterpret_cast<double *>(base + o_ex) : nullptr;
    de.c = eh->c ? reinterpret_cast<double *>(base + o_ec) : nullptr;
    de.x_off = exsel ? reinterpret_cast<const int64_t *>(base + o_exoff) : nullptr;
    halda_fleet_result r = stage::bind_result(base, R, oh);
    rc = out_h ? halda_solve_fleets_plans(ctx, model, &d, ks, n_k, &dp, &de, &r, s)
               : halda_eval_plans(ctx, model, &d, &dp, &de, s);
    const std::array<stage::Copy, 7> eval_copies = {{{eh->status, o_est, size_t(4 * nf)},
                                                     {eh->obj_value, o_eobj, size_t(8 * nf)},
                                                     {eh->cycle, o_ecyc, size_t(8 * nf)},
                                                     {eh->bottleneck, o_ebot, size_t(4 * nf)},
                                                     {eh->reason, o_erea, size_t(4 * nf)},
                                                     {eh->x, o_ex, 8 * exs},
                                                     {eh->c, o_ec, 8 * exs}}};
    if (rc == HALDA_OK) rc = download(eval_copies, base, s);
    if (rc == HALDA_OK) rc = download(stage::result_copies(R, oh), base, s);  // no sweep: every host pointer NULL
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

int halda_eval_plans_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const halda_plans *plans,
                          halda_plan_result *out) {
    const int rc = check_plans_args(ctx, model, fleets, plans, out, "halda_eval_plans_host");
    if (rc != HALDA_OK) return rc;
    return plans_host(ctx, model, fleets, nullptr, 0, plans, out, nullptr);
}

int halda_solve_fleets_plans_host(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                                  int32_t n_k, const halda_plans *plans, halda_plan_result *eval_out,
                                  halda_fleet_result *out) {
    const int rc = check_plans_args(ctx, model, fleets, plans, eval_out, "halda_solve_fleets_plans_host");
    if (rc != HALDA_OK) return rc;
    if (!ks || !out) return fail(HALDA_E_ARG, "halda_solve_fleets_plans_host: NULL ks/out");
    return plans_host(ctx, model, fleets, ks, n_k, plans, eval_out, out);
}

// ---------------------------------------------------------------- the k-sweep within per-device layer bounds
// halda_solve_fleets_bounded: every (fleet, k) instance with its w columns' bounds narrowed to
// [max(1, w_min_i), min(W, w_max_i)]. General route (the specification, every shape): fleets_csr with the
// bounds -- halda_lower_kernel, halda_bound_cols_kernel, then the screen / k = 1 / general / big kernels
// and halda_pick_kernel unchanged. Fused route: where the sweep is the register launch alone over fleets of
// one size <= kK1MaxM (kRegAlone: the sub-fleet, variants and plans kernels' gate), ONE launch of
// halda_sweep_bounds_kernel; bounds only shrink R and the set of open k, so no fleet is handed back.
// Table route (path 3 only, where the fused route does not apply): fleets of 1 .. kK1MaxM devices whose
// unbounded table slice fits the LDS budget, ONE launch of halda_sweep_bounds_tables_kernel on that slice
// (sum lo >= M, so it holds every bounded instance; nothing is handed back either).
int halda_set_bounds_path(void *ctx, int path) { return set_family_path(ctx, lrec::kBounds, path); }
int halda_last_bounds_route(void *ctx, int *route) { return last_family_route(ctx, lrec::kBounds, route); }

// halda_solve_fleets_bounded and halda_solve_fleets_boxed: one body on a halda_box (w bounds alone: its n
// arrays NULL). Without n bounds every launch is the bounded call's own kernel; with them the box kernels
// under the same gates.
static int solve_boxed(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks, int32_t n_k,
                       const halda_box &B, halda_fleet_result *out, void *stream, const char *who) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !ks || !out)
        return fail(HALDA_E_ARG, std::string(who) + ": NULL ctx/model/fleets/ks/out");
    const halda_fleets &F = *fleets;
    if (F.n_fleets <= 0) return HALDA_OK;
    {
        const int rc = check_fleets_args(model, fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    const bool nbox = B.n_min || B.n_max;
    // the fused kernels' second argument: the box kernels take all four arrays, the others the w pair
    BoundArgs Bd{B.w_min, B.w_max};
    BoxArgs Bx{B.w_min, B.w_max, B.n_min, B.n_max};
    void *bargs = nbox ? static_cast<void *>(&Bx) : static_cast<void *>(&Bd);
    // automatic = fused where admissible: one launch against the general route's lowering, patch, screen,
    // solve and pick launches
    if (c->knob[lrec::kBounds].path != 1 && c->fleets_fused && n_k <= 64) {
        SweepPlan p;
        const int rc = plan_sweep(c, *model, F, ks, n_k, *out, &p);
        if (rc != HALDA_OK) return rc;
        if (p.kind == kRegAlone && p.A.uM > 0 && p.A.uM <= kK1MaxM) {
            SweepArgs &A = p.A;
            begin_one(c, A);
            const void *fn = nbox ? reinterpret_cast<const void *>(halda_sweep_box_kernel)
                                  : reinterpret_cast<const void *>(halda_sweep_bounds_kernel);
            void *args[] = {&A, bargs};
            return launch_one(c, s, lrec::Record::reg_alone, lrec::kBounds, 1, [&]() -> int {
                HIP_TRY(hipLaunchKernel(fn, dim3(p.grid1), dim3(p.block1), args, 0, s));
                return HALDA_OK;
            });
        }
        if (c->knob[lrec::kBounds].path == 3 && F.min_devices >= 1 && F.max_devices <= kK1MaxM && p.slice <= kLdsBudget) {
            SweepArgs &A = p.A;
            begin_one(c, A);  // every fleet is solved here: nothing is flagged or handed back
            const void *fn = nbox ? reinterpret_cast<const void *>(halda_sweep_box_tables_kernel)
                                  : reinterpret_cast<const void *>(halda_sweep_bounds_tables_kernel);
            int per_cu = 0;
            HIP_TRY(c->occupancy(fn, p.slice, &per_cu));  // also raises the kernel's dynamic-LDS limit
            const unsigned grid =
                unsigned(std::max<int64_t>(1, std::min<int64_t>(int64_t(c->cus) * per_cu, int64_t(p.nf))));
            void *args[] = {&A, bargs};
            return launch_one(c, s, lrec::Record::tables_alone, lrec::kBounds, 3, [&]() -> int {
                HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(64), args, size_t(p.slice), s));
                return HALDA_OK;
            });
        }
    }
    c->knob[lrec::kBounds].route = 2;
    return fleets_csr(c, model, F, ks, n_k, out, s, &B);
}

int halda_solve_fleets_bounded(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                               int32_t n_k, const halda_bounds *bounds, halda_fleet_result *out, void *stream) {
    const halda_box B = {bounds ? bounds->w_min : nullptr, bounds ? bounds->w_max : nullptr, nullptr, nullptr};
    return solve_boxed(ctx, model, fleets, ks, n_k, B, out, stream, "halda_solve_fleets_bounded");
}

int halda_solve_fleets_boxed(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_box *box, halda_fleet_result *out, void *stream) {
    const halda_box none = {nullptr, nullptr, nullptr, nullptr};
    return solve_boxed(ctx, model, fleets, ks, n_k, box ? *box : none, out, stream, "halda_solve_fleets_boxed");
}

// The host variant: the table, the bounds (and x_off) cross PCIe once on the way in, the results on the way
// out, through the context's staging scratch.
static int solve_boxed_host(void *ctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks,
                            int32_t n_k, const halda_box &B, halda_fleet_result *out_h, const char *who) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fh || !ks || !out_h)
        return fail(HALDA_E_ARG, std::string(who) + "_host: NULL ctx/model/fleets/ks/out");
    const int64_t nf = fh->n_fleets;
    if (nf <= 0) return HALDA_OK;
    {
        const int rc = check_fleets_args(model, fh, ks, n_k, out_h);
        if (rc != HALDA_OK) return rc;
    }
    const int64_t nd = fh->dev_off[nf];
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    // layout: the table, the bounds that were passed, the results
    const int32_t *bsrc[4] = {B.w_min, B.w_max, B.n_min, B.n_max};
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    size_t o_b[4];
    for (int a = 0; a < 4; ++a) o_b[a] = bsrc[a] ? lay.take(4 * nd) : 0;
    const bool xsel = stage::compact(*out_h);
    const size_t xs = stage::xc_extent(fh->dev_off, nf, n_k, 1, fh->max_devices, xsel ? out_h->x_off : nullptr);
    const stage::ResultSlots R = stage::lay_result(lay, *out_h, nf, nd, size_t(nf) * n_k, xs);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *fh, s);
    for (int a = 0; a < 4 && rc == HALDA_OK; ++a)
        if (bsrc[a]) rc = upload(base, o_b[a], bsrc[a], 4 * nd, s);
    if (rc == HALDA_OK && xsel) rc = upload(base, R.x_off, out_h->x_off, 8 * R.n_inst, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*fh, base, T);
    auto bdev = [&](int a) { return bsrc[a] ? reinterpret_cast<const int32_t *>(base + o_b[a]) : nullptr; };
    const halda_box db = {bdev(0), bdev(1), bdev(2), bdev(3)};
    halda_fleet_result r = stage::bind_result(base, R, *out_h);
    rc = solve_boxed(ctx, model, &d, ks, n_k, db, &r, s, who);
    if (rc == HALDA_OK) rc = download(stage::result_copies(R, *out_h), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

int halda_solve_fleets_bounded_host(void *ctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks,
                                    int32_t n_k, const halda_bounds *bounds, halda_fleet_result *out_h) {
    const halda_box B = {bounds ? bounds->w_min : nullptr, bounds ? bounds->w_max : nullptr, nullptr, nullptr};
    return solve_boxed_host(ctx, model, fh, ks, n_k, B, out_h, "halda_solve_fleets_bounded");
}

int halda_solve_fleets_boxed_host(void *ctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks,
                                  int32_t n_k, const halda_box *box, halda_fleet_result *out_h) {
    const halda_box none = {nullptr, nullptr, nullptr, nullptr};
    return solve_boxed_host(ctx, model, fh, ks, n_k, box ? *box : none, out_h, "halda_solve_fleets_boxed");
}

// ---------------------------------------------------------------- one table under many boxes
// halda_solve_fleets_boxes: one fleet table under n_box boxes, the bound planes and the outputs box-major,
// slice b bit for bit what halda_solve_fleets_boxed writes for box b alone under bounds path 3.
// Loop route (the specification; every call on path 1): n_box calls of halda_solve_fleets_boxed on the
// caller's stream under bounds path 3, the bound and output pointers moved to the box's slice; the context's
// bounds path is put back before the call returns.
// Register route: under the boxed entry's fused gate, one launch of halda_sweep_boxes_kernel, blockIdx.y the
// box. Table route: else under path 3's table gate, one launch of halda_sweep_boxes_tables_kernel, its
// persistent grid over the n_box * n_fleets items. Neither uses context scratch.
int halda_set_boxes_path(void *ctx, int path) { return set_family_path(ctx, lrec::kBoxes, path); }
int halda_last_boxes_route(void *ctx, int *route) { return last_family_route(ctx, lrec::kBoxes, route); }

static int check_boxes(const halda_boxes *boxes) {
    if (!boxes) return fail(HALDA_E_ARG, "halda_solve_fleets_boxes: NULL boxes");
    if (boxes->n_box < 1 || boxes->n_box > 65535) return fail(HALDA_E_ARG, "n_box must be in 1..65535");
    return HALDA_OK;
}

// total: dev_off[n_fleets] when the caller knows it (the host variant), -1 to read it back where needed
static int solve_boxes(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks, int32_t n_k,
                       const halda_boxes *boxes, halda_fleet_result *out, void *stream, int64_t total) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !ks || !out)
        return fail(HALDA_E_ARG, "halda_solve_fleets_boxes: NULL ctx/model/fleets/ks/out");
    {
        const int rc = check_boxes(boxes);
        if (rc != HALDA_OK) return rc;
    }
    const halda_fleets &F = *fleets;
    if (F.n_fleets <= 0) return HALDA_OK;
    {
        const int rc = check_fleets_args(model, fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    const halda_boxes &B = *boxes;
    const int64_t nf = F.n_fleets, nb = B.n_box;
    // the fused kernels index fleets and (fleet, k) instances over all boxes with 32 bits
    if (c->knob[lrec::kBoxes].path == 0 && c->fleets_fused && n_k <= 64 && nb * nf * n_k < (int64_t(1) << 31)) {
        SweepPlan p;
        const int rc = plan_sweep(c, *model, F, ks, n_k, *out, &p);
        if (rc != HALDA_OK) return rc;
        const bool reg = p.kind == kRegAlone && p.A.uM > 0 && p.A.uM <= kK1MaxM;
        if (reg || (F.min_devices >= 1 && F.max_devices <= kK1MaxM && p.slice <= kLdsBudget)) {
            SweepArgs &A = p.A;
            begin_one(c, A);  // every (box, fleet) is solved in the one launch: nothing is flagged or handed back
            const BoxesArgs Bs{B.w_min, B.w_max, B.n_min, B.n_max, int(nb)};
            if (reg)
                return launch_one(c, s, lrec::Record::reg_alone, lrec::kBoxes, 1, [&]() -> int {
                    hipLaunchKernelGGL(halda_sweep_boxes_kernel, dim3(p.grid1, unsigned(nb)), dim3(p.block1), 0, s, A,
                                       Bs);
                    return launched();
                });
            const void *fn = reinterpret_cast<const void *>(halda_sweep_boxes_tables_kernel);
            int per_cu = 0;
            HIP_TRY(c->occupancy(fn, p.slice, &per_cu));  // also raises the kernel's dynamic-LDS limit
            const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(int64_t(c->cus) * per_cu, nb * nf)));
            return launch_one(c, s, lrec::Record::tables_alone, lrec::kBoxes, 3, [&]() -> int {
                hipLaunchKernelGGL(halda_sweep_boxes_tables_kernel, dim3(grid), dim3(64), size_t(p.slice), s, A, Bs);
                return launched();
            });
        }
    }
    // the loop: box b's planes in, box b's slice of every output
    int64_t nd = total;
    if (nd < 0 && nb > 1) {
        HIP_TRY(hipMemcpyAsync(&nd, F.dev_off + nf, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (nd < 0) return fail(HALDA_E_ARG, "halda_fleets: dev_off[n_fleets] < 0");
    }
    const int64_t xstride = 7 * int64_t(std::max(F.max_devices, 1)) + 1;
    const lrec::PathOverride tables(c->knob[lrec::kBounds], 3);  // (put back on return)
    c->knob[lrec::kBoxes].route = 2;
    int rc = HALDA_OK;
    for (int64_t b = 0; b < nb && rc == HALDA_OK; ++b) {
        const int64_t at = b ? b * nd : 0;
        const halda_box one = {B.w_min ? B.w_min + at : nullptr, B.w_max ? B.w_max + at : nullptr,
                               B.n_min ? B.n_min + at : nullptr, B.n_max ? B.n_max + at : nullptr};
        halda_fleet_result o = lrec::result_slice(*out, b, nf, at, n_k, xstride);
        rc = halda_solve_fleets_boxed(ctx, model, fleets, ks, n_k, &one, &o, s);
    }
    return rc;
}

int halda_solve_fleets_boxes(void *ctx, const halda_model *model, const halda_fleets *fleets, const int32_t *ks,
                             int32_t n_k, const halda_boxes *boxes, halda_fleet_result *out, void *stream) {
    return solve_boxes(ctx, model, fleets, ks, n_k, boxes, out, stream, -1);
}

// The host variant: the table crosses PCIe once, the bound planes that were passed once, and the n_box result
// slices come back, through the context's staging scratch. It knows dev_off[n_fleets]: no read-back.
int halda_solve_fleets_boxes_host(void *ctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks,
                                  int32_t n_k, const halda_boxes *boxes, halda_fleet_result *out_h) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fh || !ks || !out_h)
        return fail(HALDA_E_ARG, "halda_solve_fleets_boxes_host: NULL ctx/model/fleets/ks/out");
    {
        const int rc = check_boxes(boxes);
        if (rc != HALDA_OK) return rc;
    }
    const int64_t nf = fh->n_fleets, nb = boxes->n_box;
    if (nf <= 0) return HALDA_OK;
    {
        const int rc = check_fleets_args(model, fh, ks, n_k, out_h);
        if (rc != HALDA_OK) return rc;
    }
    const int64_t nd = fh->dev_off[nf];
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    // layout: the table, once; the planes that were passed; the results box-major over (box, fleet, k)
    const int32_t *bsrc[4] = {boxes->w_min, boxes->w_max, boxes->n_min, boxes->n_max};
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    size_t o_b[4];
    for (int a = 0; a < 4; ++a) o_b[a] = bsrc[a] ? lay.take(4 * nb * nd) : 0;
    const bool xsel = stage::compact(*out_h);
    const size_t xs = stage::xc_extent(fh->dev_off, nf, n_k, nb, fh->max_devices, xsel ? out_h->x_off : nullptr);
    const stage::ResultSlots R = stage::lay_result(lay, *out_h, nb * nf, nb * nd, size_t(nb) * nf * n_k, xs);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *fh, s);
    for (int a = 0; a < 4 && rc == HALDA_OK; ++a)
        if (bsrc[a]) rc = upload(base, o_b[a], bsrc[a], 4 * nb * nd, s);
    if (rc == HALDA_OK && xsel) rc = upload(base, R.x_off, out_h->x_off, 8 * R.n_inst, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*fh, base, T);
    auto bdev = [&](int a) { return bsrc[a] ? reinterpret_cast<const int32_t *>(base + o_b[a]) : nullptr; };
    const halda_boxes db = {boxes->n_box, bdev(0), bdev(1), bdev(2), bdev(3)};
    halda_fleet_result r = stage::bind_result(base, R, *out_h);
    rc = solve_boxes(ctx, model, &d, ks, n_k, &db, &r, s, nd);
    if (rc == HALDA_OK) rc = download(stage::result_copies(R, *out_h), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- the frontier launches (budget and change)
// Both entries run ONE launch of their kernel under a gate formed from the shapes alone. No context scratch,
// no flags, nothing handed back; outside the gate an error and no launch.
constexpr int kBudgetMaxP = 63;

// The gate's common part, in the order both entries report it: the table, the model, k, the incumbent array,
// the result arrays, 1 .. kK1MaxM devices per fleet / list, max_p. `in` / `out` / `unit` name the entry's
// input struct, result struct and what a row of devices is called.
static int check_frontier_gate(const halda_fleets &table, const halda_model &model, int32_t k, bool has_w0,
                               bool has_out, int min_devices, int max_devices, int max_p, const std::string &who,
                               const char *in, const char *out, const char *unit) {
    if (!stage::complete(table)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    if (model.L < 1) return fail(HALDA_E_ARG, "model.L < 1");
    if (k < 1) return fail(HALDA_E_ARG, who + ": k must be >= 1");
    if (!has_w0) return fail(HALDA_E_ARG, who + ": " + in + ".w0 is NULL");
    if (!has_out) return fail(HALDA_E_ARG, who + ": " + out + " has a NULL array");
    if (min_devices < 1 || max_devices < min_devices || max_devices > kK1MaxM)
        return fail(HALDA_E_ARG, who + ": every " + unit + " must have 1 .. 64 devices");
    if (max_p < 0 || max_p > kBudgetMaxP) return fail(HALDA_E_ARG, who + ": max_p must be in 0 .. 63");
    return HALDA_OK;
}

static int check_frontier_lds(int64_t lds, const std::string &who) {
    if (lds > kLdsBudget)
        return fail(HALDA_E_ARG, who + ": the slice of " + std::to_string(lds) + " B exceeds the LDS budget of " +
                                     std::to_string(kLdsBudget) + " B");
    return HALDA_OK;
}

// ---------------------------------------------------------------- a total move budget and its frontier
// halda_solve_fleets_budget: halda_sweep_budget_kernel; the gate is fleets of 1 .. kK1MaxM devices, one k,
// max_p <= 63, the slice within the LDS budget.
int64_t halda_budget_lds_bytes(int32_t max_devices, int32_t max_p, int32_t k) {
    if (max_devices < 1 || max_p < 0 || k < 1) return -1;
    if (max_devices > 4096 || max_p > 4096) return INT64_MAX;  // far outside the gate; no overflow below
    return budget_slice(max_devices, max_p, k > 1).total;
}

static int check_budget_args(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                             const halda_budget *budget, const halda_frontier *fr, const char *who) {
    if (!ctx || !model || !fleets || !budget || !fr)
        return fail(HALDA_E_ARG, std::string(who) + ": NULL ctx/model/fleets/budget/frontier");
    const halda_fleets &F = *fleets;
    if (F.n_fleets <= 0) return HALDA_OK;
    const int rc = check_frontier_gate(F, *model, k, budget->w0, fr->status && fr->obj && fr->moved && fr->w && fr->n,
                                       F.min_devices, F.max_devices, budget->max_p, who, "halda_budget",
                                       "halda_frontier", "fleet");
    if (rc != HALDA_OK) return rc;
    return check_frontier_lds(halda_budget_lds_bytes(F.max_devices, budget->max_p, k), who);
}

int halda_solve_fleets_budget(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                              const halda_budget *budget, halda_frontier *frontier, void *stream) {
    const int rc = check_budget_args(ctx, model, fleets, k, budget, frontier, "halda_solve_fleets_budget");
    if (rc != HALDA_OK) return rc;
    const halda_fleets &F = *fleets;
    if (F.n_fleets <= 0) return HALDA_OK;
    if (frontier->n_devices < F.n_fleets)
        return fail(HALDA_E_ARG, "halda_solve_fleets_budget: halda_frontier.n_devices is not dev_off[n_fleets]");
    const BudgetArgs Bg{budget->w0,       budget->w_min,   budget->w_max,   budget->max_p, frontier->n_devices,
                        frontier->status, frontier->obj,   frontier->moved, frontier->w,   frontier->n};
    return launch_frontier(static_cast<Ctx *>(ctx), halda_sweep_budget_kernel, *model, F, k,
                           budget_slice(F.max_devices, budget->max_p, k > 1).total, Bg, stream);
}

int halda_solve_fleets_budget_host(void *ctx, const halda_model *model, const halda_fleets *fh, int32_t k,
                                   const halda_budget *budget, halda_frontier *fr_h) {
    int rc = check_budget_args(ctx, model, fh, k, budget, fr_h, "halda_solve_fleets_budget_host");
    if (rc != HALDA_OK) return rc;
    Ctx *c = static_cast<Ctx *>(ctx);
    const int64_t nf = fh->n_fleets;
    if (nf <= 0) return HALDA_OK;
    const int64_t nd = fh->dev_off[nf];
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    {
        const int64_t f = stage::bad_incumbent(fh->dev_off, nf, budget->w0, model->L / k);
        if (f >= 0)
            return fail(HALDA_E_ARG, "halda_solve_fleets_budget_host: fleet " + std::to_string(f) +
                                         ": the incumbent needs every w0_i >= 1 and sum w0 = L / k");
    }
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const stage::TripleLayout B = stage::lay_triple(lay, budget->w0, budget->w_min, budget->w_max, nd);
    const stage::FrontierSlots R = stage::lay_frontier(lay, nf, nd, budget->max_p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *fh, s);
    if (rc == HALDA_OK) rc = upload(base, B, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*fh, base, T);
    const halda_budget db = {B.at(base, 0), B.at(base, 1), B.at(base, 2), budget->max_p};
    halda_frontier r = stage::bind_frontier(base, R, nd);
    rc = halda_solve_fleets_budget(ctx, model, &d, k, &db, &r, s);
    if (rc == HALDA_OK) rc = download(stage::frontier_copies(R, *fr_h), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- a changed fleet and its frontier
// halda_solve_change: halda_sweep_change_kernel; the gate is lists of 1 .. kK1MaxM devices, one k,
// max_p <= 63, 2 max_p + max_deficit <= 254, the slice within the LDS budget.
constexpr int kChangeMaxE = 254;  // the arg-min byte: table entries 0 .. 2 P + D, 255 marks "unreached"

int64_t halda_change_lds_bytes(int32_t max_devices, int32_t max_p, int32_t max_deficit, int32_t k) {
    if (max_devices < 1 || max_p < 0 || max_deficit < 0 || k < 1) return -1;
    if (max_devices > 4096 || max_p > 4096 || max_deficit > 65536) return INT64_MAX;  // far outside the gate
    return change_slice(max_devices, max_p, max_deficit, k > 1).total;
}

static int check_change_args(void *ctx, const halda_model *model, const halda_fleets *table,
                             const halda_subfleets *items, int32_t k, const halda_change *change,
                             const halda_change_frontier *fr, bool host, const char *who) {
    if (!ctx || !model || !table || !items || !change || !fr)
        return fail(HALDA_E_ARG, std::string(who) + ": NULL ctx/model/table/items/change/frontier");
    const halda_subfleets &I = *items;
    if (I.n_items <= 0) return HALDA_OK;
    if (!I.parent || !I.sub_off || !I.sub_idx) return fail(HALDA_E_ARG, "halda_subfleets has a NULL array");
    if (table->n_fleets <= 0) return fail(HALDA_E_ARG, std::string(who) + ": the table has no fleets");
    const int rc = check_frontier_gate(*table, *model, k, change->w0,
                                       fr->status && fr->obj && fr->loaded && fr->released && fr->w && fr->n,
                                       I.min_devices, I.max_devices, change->max_p, who, "halda_change",
                                       "halda_change_frontier", "list");
    if (rc != HALDA_OK) return rc;
    if (change->max_deficit < (host ? -1 : 0))
        return fail(HALDA_E_ARG, std::string(who) + ": max_deficit must be >= 0");
    const int dmax = std::max(change->max_deficit, 0);
    if (2 * int64_t(change->max_p) + dmax > kChangeMaxE)
        return fail(HALDA_E_ARG, std::string(who) + ": 2 max_p + max_deficit must be at most 254");
    return check_frontier_lds(halda_change_lds_bytes(I.max_devices, change->max_p, dmax, k), who);
}

int halda_solve_change(void *ctx, const halda_model *model, const halda_fleets *table, const halda_subfleets *items,
                       int32_t k, const halda_change *change, halda_change_frontier *frontier, void *stream) {
    const int rc = check_change_args(ctx, model, table, items, k, change, frontier, false, "halda_solve_change");
    if (rc != HALDA_OK) return rc;
    const halda_subfleets &I = *items;
    if (I.n_items <= 0) return HALDA_OK;
    if (frontier->n_devices < I.n_items)
        return fail(HALDA_E_ARG, "halda_solve_change: halda_change_frontier.n_devices is not sub_off[n_items]");
    halda_fleets view = *table;  // the parent table under the items' count and length summary
    view.n_fleets = I.n_items;
    view.min_devices = I.min_devices;
    view.max_devices = I.max_devices;
    const ChangeArgs Cg{SubArgs{I.parent, I.sub_off, I.sub_idx},
                        change->w0,
                        change->w_min,
                        change->w_max,
                        change->max_p,
                        change->max_deficit,
                        frontier->n_devices,
                        frontier->status,
                        frontier->obj,
                        frontier->loaded,
                        frontier->released,
                        frontier->w,
                        frontier->n};
    return launch_frontier(static_cast<Ctx *>(ctx), halda_sweep_change_kernel, *model, view, k,
                           change_slice(I.max_devices, change->max_p, change->max_deficit, k > 1).total, Cg, stream);
}

int halda_solve_change_host(void *ctx, const halda_model *model, const halda_fleets *th, const halda_subfleets *ih,
                            int32_t k, const halda_change *change, halda_change_frontier *fr_h) {
    const char *who = "halda_solve_change_host";
    if (!ctx || !model || !th || !ih || !change || !fr_h)
        return fail(HALDA_E_ARG, std::string(who) + ": NULL ctx/model/table/items/change/frontier");
    Ctx *c = static_cast<Ctx *>(ctx);
    const int64_t n = ih->n_items;
    if (n <= 0) return HALDA_OK;
    if (!ih->parent || !ih->sub_off || !ih->sub_idx) return fail(HALDA_E_ARG, "halda_subfleets has a NULL array");
    if (th->n_fleets <= 0 || !th->dev_off) return fail(HALDA_E_ARG, std::string(who) + ": empty table");
    const int64_t nf = th->n_fleets, nd = th->dev_off[nf];
    if (nd < nf) return fail(HALDA_E_ARG, "bad device count");
    int64_t lmin = 0, lmax = 0;
    int rc = check_items_host(*th, *ih, &lmin, &lmax);
    if (rc != HALDA_OK) return rc;
    if ((ih->min_devices || ih->max_devices) && (lmin != ih->min_devices || lmax != ih->max_devices))
        return fail(HALDA_E_ARG, "halda_subfleets: min_devices / max_devices are not the lists' shortest and longest "
                                 "length (" + std::to_string(lmin) + ", " + std::to_string(lmax) + ")");
    halda_subfleets di = *ih;
    di.min_devices = int32_t(std::min<int64_t>(lmin, INT32_MAX));
    di.max_devices = int32_t(std::min<int64_t>(lmax, INT32_MAX));
    rc = check_change_args(ctx, model, th, &di, k, change, fr_h, true, who);
    if (rc != HALDA_OK) return rc;
    // the incumbents: every w0_i >= 0 and 0 <= D <= max_deficit (-1: the items' largest D is taken)
    int64_t dtop = 0;
    {
        const int64_t i = stage::bad_change(ih->sub_off, n, change->w0, model->L / k, change->max_deficit, &dtop);
        if (i >= 0)
            return fail(HALDA_E_ARG, std::string(who) + ": item " + std::to_string(i) +
                                         ": needs every w0_i >= 0 and a deficit L / k - sum w0 in 0 .. max_deficit");
    }
    halda_change dc = *change;
    if (dc.max_deficit < 0) {
        if (dtop > kChangeMaxE) return fail(HALDA_E_ARG, std::string(who) + ": 2 max_p + max_deficit must be at most 254");
        dc.max_deficit = int32_t(dtop);
        rc = check_change_args(ctx, model, th, &di, k, &dc, fr_h, true, who);
        if (rc != HALDA_OK) return rc;
    }
    const int64_t tot = ih->sub_off[n];
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const stage::ItemsLayout IL = stage::lay_items(lay, n, tot);
    const stage::TripleLayout B = stage::lay_triple(lay, change->w0, change->w_min, change->w_max, tot);
    const stage::ChangeSlots R = stage::lay_change(lay, n, tot, dc.max_p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *th, s);
    if (rc == HALDA_OK) rc = upload(base, IL, *ih, s);
    if (rc == HALDA_OK) rc = upload(base, B, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*th, base, T);
    di = stage::rebase(di, base, IL);
    dc.w0 = B.at(base, 0);
    dc.w_min = B.at(base, 1);
    dc.w_max = B.at(base, 2);
    halda_change_frontier r = stage::bind_change(base, R, tot);
    rc = halda_solve_change(ctx, model, &d, &di, k, &dc, &r, s);
    if (rc == HALDA_OK) rc = download(stage::change_copies(R, *fr_h), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- scale-in / scale-out
// halda_solve_change_subsets: halda_solve_subsets' candidates (the same combo lists and per-(d, fleet)
// records) under halda_solve_change's value. Per d one or more launches, each of its d's list lengths and
// max_deficit = that d's largest deficit: index kernel, halda_solve_change on the items just written, pick
// kernel. A launch's scratch (halda_change_subsets_launch_bytes) stays within the context's cap; everything
// lives in the context's grow-only sel_buf, so the call runs after the previous user of the context's shared
// scratch on another stream (order_after_previous).
constexpr int64_t kChangeSubsetsChunkBytes = int64_t(256) << 20;
constexpr int64_t kChangeSubsetsFixedBytes = 4096;  // the launch's 12 regions, each 256-byte aligned, and sub_off's end

static int64_t change_subsets_item_bytes(int len, int P1) {
    // parent, sub_off, the four per-point arrays; per listed device sub_idx, w0 / w_min / w_max and the two planes
    return 12 + 20 * int64_t(P1) + int64_t(len) * (16 + 8 * int64_t(P1));
}

int64_t halda_change_subsets_launch_bytes(int32_t len, int32_t max_p, int64_t n_items) {
    if (len < 1 || max_p < 0 || n_items < 0) return -1;
    return kChangeSubsetsFixedBytes + n_items * change_subsets_item_bytes(len, max_p + 1);
}

int halda_set_change_subsets_chunk(void *ctx, int64_t bytes) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c) return fail(HALDA_E_ARG, "NULL ctx");
    if (bytes < 0) return fail(HALDA_E_ARG, "the chunk cap must be >= 0 (0: the default)");
    c->scale_chunk = bytes;
    return HALDA_OK;
}

int64_t halda_change_subsets_max_deficit(const int32_t *w0, int32_t M, uint64_t keep_mask, int32_t d, int32_t W) {
    if (!w0 || M < 1 || M > 64 || d < 0) return -1;
    const uint64_t all = M == 64 ? ~uint64_t(0) : (uint64_t(1) << M) - 1;
    if (keep_mask & ~all) return -1;
    int64_t sum = 0;
    std::vector<int64_t> can;
    for (int i = 0; i < M; ++i) {
        sum += w0[i];
        if (!((keep_mask >> i) & 1)) can.push_back(w0[i]);
    }
    if (d > int(can.size())) return -1;
    std::sort(can.begin(), can.end(), std::greater<int64_t>());
    int64_t D = int64_t(W) - sum;
    for (int j = 0; j < d; ++j) D += can[j];
    return D;
}

// The gate's findings: per fleet its droppable devices, their count, the most it may drop within the range and
// its size; per d of the range the largest deficit and the longest list of the fleets that admit it (-1 / 0: none).
struct ChangeSubsetsGate {
    std::vector<uint64_t> drop;
    std::vector<int> qs, Df, sizes;
    std::vector<int64_t> dtop;
    std::vector<int> ltop;
};

// The gate, from the shapes and w0 alone: no GPU work. off / w0_h: the table's dev_off and the call's w0 in HOST
// memory.
static int change_subsets_gate(const halda_model *model, const halda_fleets *table, const int64_t *off,
                               const int32_t *w0_h, int32_t k, const halda_change_subsets *cs,
                               const halda_change_subset_frontier *fr, ChangeSubsetsGate &Q) {
    const char *who = "halda_solve_change_subsets";
    const int nf = table->n_fleets, d0 = cs->min_drop, d1 = cs->max_drop, P = cs->max_p;
    const uint64_t *keep = cs->keep_mask;
    if (!fr->status || !fr->obj || !fr->dropped_mask || !fr->loaded || !fr->released || !fr->w || !fr->n)
        return fail(HALDA_E_ARG, "halda_change_subset_frontier has a NULL array");
    if (!cs->w0) return fail(HALDA_E_ARG, "halda_change_subsets.w0 is NULL");
    if (d0 < 0 || d1 < d0 || d1 > 63)
        return fail(HALDA_E_ARG, std::string(who) + ": needs 0 <= min_drop <= max_drop <= 63");
    if (P < 0 || P > kBudgetMaxP) return fail(HALDA_E_ARG, std::string(who) + ": max_p must be in 0 .. 63");
    if (model->L < 1) return fail(HALDA_E_ARG, "model.L < 1");
    if (k < 1) return fail(HALDA_E_ARG, std::string(who) + ": k must be >= 1");
    if (!stage::complete(*table)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    // the gate, from the shapes and w0 alone
    const int64_t W = model->L / k;
    const int D1 = d1 - d0 + 1;
    std::vector<uint64_t> &drop = Q.drop;
    std::vector<int> &qs = Q.qs, &Df = Q.Df, &sizes = Q.sizes, &ltop = Q.ltop;
    std::vector<int64_t> &dtop = Q.dtop;
    drop.assign(nf, 0);
    qs.assign(nf, 0);
    Df.assign(nf, 0);
    sizes.assign(nf, 0);
    dtop.assign(size_t(D1), -1);
    ltop.assign(size_t(D1), 0);
    bool any = false;
    for (int f = 0; f < nf; ++f) {
        const int64_t M64 = off[f + 1] - off[f];
        if (M64 < 1 || M64 > 64)
            return fail(HALDA_E_ARG, std::string(who) + ": fleet " + std::to_string(f) + " has " + std::to_string(M64) +
                                         " devices (1..64)");
        const int M = sizes[f] = int(M64);
        const uint64_t all = M == 64 ? ~uint64_t(0) : (uint64_t(1) << M) - 1, km = keep ? keep[f] : 0;
        if (km & ~all)
            return fail(HALDA_E_ARG, "halda_change_subsets: keep_mask of fleet " + std::to_string(f) +
                                         " names a device past " + std::to_string(M));
        drop[f] = all & ~km;
        qs[f] = __builtin_popcountll(drop[f]);
        Df[f] = std::min({d1, qs[f], M - 1});
        int64_t sum = 0, cnt = 0;
        std::vector<int64_t> can;
        for (int i = 0; i < M; ++i) {
            const int64_t v = w0_h[off[f] + i];
            if (v < 0)
                return fail(HALDA_E_ARG, std::string(who) + ": fleet " + std::to_string(f) + ": every w0_i must be >= 0");
            sum += v;
            if ((drop[f] >> i) & 1) can.push_back(v);
        }
        if (sum > W)
            return fail(HALDA_E_ARG, std::string(who) + ": fleet " + std::to_string(f) + ": w0 sums to " +
                                         std::to_string(sum) + ", above L / k = " + std::to_string(W));
        std::sort(can.begin(), can.end(), std::greater<int64_t>());
        int64_t D = W - sum;
        for (int d = 0; d <= Df[f]; ++d) {
            if (d) D += can[d - 1];
            if (d < d0) continue;
            any = true;
            cnt += binom_sat(qs[f], d);
            if (cnt > HALDA_SUBSETS_MAX)
                return fail(HALDA_E_ARG, std::string(who) + ": fleet " + std::to_string(f) + " has more than " +
                                             std::to_string(HALDA_SUBSETS_MAX) + " candidates");
            dtop[d - d0] = std::max(dtop[d - d0], D);
            ltop[d - d0] = std::max(ltop[d - d0], M - d);
        }
    }
    if (!any)
        return fail(HALDA_E_ARG, "halda_change_subsets: min_drop " + std::to_string(d0) +
                                     " is beyond min(q, M - 1) of every fleet");
    for (int j = 0; j < D1; ++j) {
        if (dtop[j] < 0) continue;
        if (2 * int64_t(P) + dtop[j] > kChangeMaxE)
            return fail(HALDA_E_ARG, std::string(who) + ": d = " + std::to_string(d0 + j) + ": 2 max_p + deficit = " +
                                         std::to_string(2 * int64_t(P) + dtop[j]) + " must be at most 254");
        const int64_t lds = halda_change_lds_bytes(ltop[j], P, int32_t(dtop[j]), k);
        if (lds > kLdsBudget)
            return fail(HALDA_E_ARG, std::string(who) + ": d = " + std::to_string(d0 + j) + ": the slice of " +
                                         std::to_string(lds) + " B exceeds the LDS budget of " +
                                         std::to_string(kLdsBudget) + " B");
    }
    return HALDA_OK;
}

// table, cs->w0 / w_min / w_max and fr hold device arrays; Q: the call's gate, passed
static int solve_change_subsets(void *ctx, const halda_model *model, const halda_fleets *table, int32_t k,
                                const halda_change_subsets *cs, halda_change_subset_frontier *fr,
                                const ChangeSubsetsGate &Q, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    const int nf = table->n_fleets, d0 = cs->min_drop, d1 = cs->max_drop, P = cs->max_p;
    const int D1 = d1 - d0 + 1, P1 = P + 1;
    const std::vector<uint64_t> &drop = Q.drop;
    const std::vector<int> &qs = Q.qs, &Df = Q.Df, &sizes = Q.sizes;
    const std::vector<int64_t> &dtop = Q.dtop;
    hipStream_t s = nullptr;
    if (const int rc = enter(c, stream, &s)) return rc;
    // the combo lists of every (q, d) in use, the records per (d, fleet), the launches
    const int64_t cap = c->scale_chunk > 0 ? c->scale_chunk : kChangeSubsetsChunkBytes;
    std::vector<uint64_t> combos;
    std::vector<int64_t> coff(65 * 64, -1);
    std::vector<SubsetFleet> recs(size_t(D1) * nf);
    std::vector<SubsetLaunch> launches;
    int64_t max_items = 0, max_dev = 0;
    for (int d = d0; d <= d1; ++d) {
        SubsetFleet *R = recs.data() + size_t(d - d0) * nf;
        int64_t items = 0, devs = 0;
        for (int f = 0; f < nf; ++f) {
            SubsetFleet &r = R[f];
            r = SubsetFleet{};
            r.drop_mask = drop[f];
            r.M = sizes[f];
            r.cnt = d <= Df[f] ? int32_t(binom_sat(qs[f], d)) : 0;
            if (r.cnt > 0) {
                int64_t &o = coff[size_t(qs[f]) * 64 + d];
                if (o < 0) {
                    o = int64_t(combos.size());
                    subset_combos(qs[f], d, combos);
                }
                r.combo_off = o;
            }
            r.item_off = items;
            r.list_off = devs;
            items += r.cnt;
            devs += int64_t(r.cnt) * (sizes[f] - d);
        }
        if (items == 0) {  // no fleet admits this d: the pick alone, which writes the empty cells
            launches.push_back(SubsetLaunch{d, false, 0, 0, 0, 0, 0, 0});
            continue;
        }
        // chunks within the byte cap, cut at candidate boundaries (one candidate at the least)
        int f = 0;
        int64_t a = 0;
        while (a < items) {
            SubsetLaunch L{d, false, a, 0, 0, 0, 64, 0};
            while (R[f].cnt == 0 || R[f].item_off + R[f].cnt <= a) ++f;
            L.l0 = R[f].list_off + (a - R[f].item_off) * (sizes[f] - d);
            int64_t b = a, bytes = kChangeSubsetsFixedBytes;
            for (int g = f; g < nf && b < items; ++g) {
                if (R[g].cnt == 0) continue;
                const int len = sizes[g] - d;
                const int64_t left = R[g].item_off + R[g].cnt - b, each = change_subsets_item_bytes(len, P1);
                int64_t take = std::min<int64_t>(left, (cap - bytes) / each);
                if (take <= 0 && L.n == 0) take = 1;
                if (take <= 0) break;
                take = std::min<int64_t>(take, (INT32_MAX / 2) / P1 - L.n);
                L.n += take;
                L.nd += take * len;
                bytes += take * each;
                L.lmin = std::min(L.lmin, len);
                L.lmax = std::max(L.lmax, len);
                b += take;
                if (take < left) break;
            }
            launches.push_back(L);
            max_items = std::max(max_items, L.n);
            max_dev = std::max(max_dev, L.nd);
            a = b;
        }
    }
    stage::Bump lay;
    const size_t pts = size_t(max_items) * P1, pl = size_t(max_dev) * P1;
    const size_t o_combo = lay.take(8 * combos.size()), o_rec = lay.take(sizeof(SubsetFleet) * recs.size()),
                 o_par = lay.take(4 * size_t(max_items)), o_soff = lay.take(8 * size_t(max_items + 1)),
                 o_sidx = lay.take(4 * size_t(max_dev)), o_w0 = lay.take(4 * size_t(max_dev)),
                 o_lo = lay.take(4 * size_t(max_dev)), o_hi = lay.take(4 * size_t(max_dev)), o_st = lay.take(4 * pts),
                 o_obj = lay.take(8 * pts), o_ld = lay.take(4 * pts), o_rl = lay.take(4 * pts), o_w = lay.take(4 * pl),
                 o_n = lay.take(4 * pl);
    {
        int rc = order_after_previous(c, s);
        if (rc == HALDA_OK) rc = grow(&c->sel_buf, &c->sel_bytes, lay.off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = reinterpret_cast<char *>(c->sel_buf);
    // (pageable sources: the copies are staged before the calls return)
    if (!combos.empty())
        HIP_TRY(hipMemcpyAsync(base + o_combo, combos.data(), 8 * combos.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + o_rec, recs.data(), sizeof(SubsetFleet) * recs.size(), hipMemcpyHostToDevice, s));
    auto i32 = [&](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
    const ChangeSubsetsSrc G{table->dev_off, cs->w0, cs->w_min, cs->w_max};
    const ChangeSubsetsItems O{i32(o_par), reinterpret_cast<int64_t *>(base + o_soff), i32(o_sidx), i32(o_w0), i32(o_lo),
                               i32(o_hi)};
    const ChangeSubsetGrid GR{fr->status, fr->obj, fr->dropped_mask, fr->loaded, fr->released, fr->w, fr->n};
    for (const SubsetLaunch &L : launches) {
        SubsetArgs U = {};
        U.fl = reinterpret_cast<const SubsetFleet *>(base + o_rec) + size_t(L.d - d0) * nf;
        U.combos = reinterpret_cast<const uint64_t *>(base + o_combo);
        U.i0 = L.i0;
        U.l0 = L.l0;
        U.n = int32_t(L.n);
        U.n_fleets = nf;
        U.d = L.d;
        if (L.n > 0) {
            hipLaunchKernelGGL(halda_change_subsets_index_kernel, dim3(unsigned((L.n + 3) / 4)), dim3(256), 0, s, U, G, O);
            HIP_TRY(hipGetLastError());
            // halda_solve_change, unedited, on the items just written
            halda_subfleets I;
            I.n_items = int32_t(L.n);
            I.min_devices = L.lmin;
            I.max_devices = L.lmax;
            I.parent = O.parent;
            I.sub_off = O.sub_off;
            I.sub_idx = O.sub_idx;
            const halda_change ch{O.w0, cs->w_min ? O.w_min : nullptr, cs->w_max ? O.w_max : nullptr, P,
                                  int32_t(dtop[L.d - d0])};
            halda_change_frontier cf;
            cf.n_devices = L.nd;
            cf.status = i32(o_st);
            cf.obj = reinterpret_cast<double *>(base + o_obj);
            cf.loaded = i32(o_ld);
            cf.released = i32(o_rl);
            cf.w = i32(o_w);
            cf.n = i32(o_n);
            const int rc = halda_solve_change(ctx, model, table, &I, k, &ch, &cf, s);
            if (rc != HALDA_OK) return rc;
        }
        const ChangeSubsetsChunk C{reinterpret_cast<const double *>(base + o_obj), i32(o_ld), i32(o_rl), i32(o_w), i32(o_n),
                                   L.nd, P1, D1, d0};
        hipLaunchKernelGGL(halda_change_subsets_pick_kernel, dim3(unsigned(nf)), dim3(256), 0, s, U, C, GR);
        HIP_TRY(hipGetLastError());
    }
    return HALDA_OK;
}

int halda_solve_change_subsets(void *ctx, const halda_model *model, const halda_fleets *fleets, int32_t k,
                               const halda_change_subsets *subsets, halda_change_subset_frontier *frontier,
                               void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !subsets || !frontier)
        return fail(HALDA_E_ARG, "NULL ctx/model/fleets/subsets/frontier");
    const int64_t nf = fleets->n_fleets;
    if (nf <= 0) return HALDA_OK;
    if (!fleets->dev_off) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    if (!subsets->w0) return fail(HALDA_E_ARG, "halda_change_subsets.w0 is NULL");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    // the gate reads dev_off and w0: both come back once
    std::vector<int64_t> off(size_t(nf) + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), fleets->dev_off, 8 * (nf + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (off[0] != 0) return fail(HALDA_E_ARG, "halda_solve_change_subsets: dev_off[0] must be 0");
    for (int64_t f = 0; f < nf; ++f)
        if (off[f + 1] - off[f] < 1 || off[f + 1] - off[f] > 64)
            return fail(HALDA_E_ARG, "halda_solve_change_subsets: fleet " + std::to_string(f) + " has " +
                                         std::to_string(off[f + 1] - off[f]) + " devices (1..64)");
    std::vector<int32_t> w0(static_cast<size_t>(off[nf]), 0);
    HIP_TRY(hipMemcpyAsync(w0.data(), subsets->w0, 4 * size_t(off[nf]), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ChangeSubsetsGate Q;
    const int rc = change_subsets_gate(model, fleets, off.data(), w0.data(), k, subsets, frontier, Q);
    if (rc != HALDA_OK) return rc;
    return solve_change_subsets(ctx, model, fleets, k, subsets, frontier, Q, stream);
}

int halda_solve_change_subsets_host(void *ctx, const halda_model *model, const halda_fleets *th, int32_t k,
                                    const halda_change_subsets *subsets, halda_change_subset_frontier *fh) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !th || !subsets || !fh) return fail(HALDA_E_ARG, "NULL ctx/model/fleets/subsets/frontier");
    if (th->n_fleets <= 0) return HALDA_OK;
    if (!stage::complete(*th)) return fail(HALDA_E_ARG, "halda_fleets has a NULL array");
    if (!fh->status || !fh->obj || !fh->dropped_mask || !fh->loaded || !fh->released || !fh->w || !fh->n)
        return fail(HALDA_E_ARG, "halda_change_subset_frontier has a NULL array");
    if (!subsets->w0) return fail(HALDA_E_ARG, "halda_change_subsets.w0 is NULL");
    if (subsets->min_drop < 0 || subsets->max_drop < subsets->min_drop || subsets->max_drop > 63)
        return fail(HALDA_E_ARG, "halda_solve_change_subsets_host: needs 0 <= min_drop <= max_drop <= 63");
    if (subsets->max_p < 0 || subsets->max_p > kBudgetMaxP)
        return fail(HALDA_E_ARG, "halda_solve_change_subsets_host: max_p must be in 0 .. 63");
    const int64_t nf = th->n_fleets, nd = th->dev_off[nf];
    if (th->dev_off[0] != 0 || nd < nf) return fail(HALDA_E_ARG, "bad device count");
    for (int64_t f = 0; f < nf; ++f)
        if (th->dev_off[f + 1] - th->dev_off[f] < 1 || th->dev_off[f + 1] - th->dev_off[f] > 64)
            return fail(HALDA_E_ARG, "halda_solve_change_subsets_host: fleet " + std::to_string(f) + " has " +
                                         std::to_string(th->dev_off[f + 1] - th->dev_off[f]) + " devices (1..64)");
    ChangeSubsetsGate Q;
    int rc = change_subsets_gate(model, th, th->dev_off, subsets->w0, k, subsets, fh, Q);
    if (rc != HALDA_OK) return rc;
    const size_t pts = size_t(nf) * size_t(subsets->max_drop - subsets->min_drop + 1) * size_t(subsets->max_p + 1);
    stage::Bump lay;
    const stage::TableLayout T = stage::lay_table(lay, nf, nd);
    const stage::TripleLayout B = stage::lay_triple(lay, subsets->w0, subsets->w_min, subsets->w_max, nd);
    const stage::ChangeSubsetSlots R = stage::lay_change_subsets(lay, pts);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    rc = ensure_scratch(c, lay.off);
    char *base = static_cast<char *>(c->scratch);
    if (rc == HALDA_OK) rc = upload(base, T, *th, s);
    if (rc == HALDA_OK) rc = upload(base, B, s);
    if (rc != HALDA_OK) return rc;
    const halda_fleets d = stage::rebase(*th, base, T);
    halda_change_subsets dc = *subsets;
    dc.w0 = B.at(base, 0);
    dc.w_min = B.at(base, 1);
    dc.w_max = B.at(base, 2);
    halda_change_subset_frontier r = stage::bind_change_subsets(base, R);
    rc = solve_change_subsets(ctx, model, &d, k, &dc, &r, Q, s);
    if (rc == HALDA_OK) rc = download(stage::change_subsets_copies(R, *fh), base, s);
    if (rc != HALDA_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

// ---------------------------------------------------------------- several GPUs, one process
// The fleets of one call are independent: a multi-device context deals them out in contiguous
// blocks, one host thread per device runs halda_solve_fleets_host on its block, and the results
// land in the caller's arrays at the block's offsets. No collective is needed (the argmin over k is
// per fleet, on the device that solved it); multi-process / multi-node callers use one halda_init
// context per rank and torch.distributed / RCCL around it (distilp_amd/distributed.py).
struct MultiCtx {
    std::vector<void *> ctxs;
};

int halda_init_multi(int n_dev, const int *ordinals, void **mctx) {
    if (!mctx || n_dev < 1 || n_dev > 64 || !ordinals) return fail(HALDA_E_ARG, "halda_init_multi: bad arguments");
    MultiCtx *m = new MultiCtx();
    for (int i = 0; i < n_dev; ++i) {
        void *c = nullptr;
        const int rc = halda_init(ordinals[i], &c);
        if (rc != HALDA_OK) {
            for (void *o : m->ctxs) halda_free(o);
            delete m;
            return rc;
        }
        m->ctxs.push_back(c);
    }
    *mctx = m;
    return HALDA_OK;
}

void halda_free_multi(void *mctx) {
    MultiCtx *m = static_cast<MultiCtx *>(mctx);
    if (!m) return;
    for (void *c : m->ctxs) halda_free(c);
    delete m;
}

int halda_solve_fleets_multi(void *mctx, const halda_model *model, const halda_fleets *fh, const int32_t *ks,
                             int32_t n_k, halda_fleet_result *out_h) {
    MultiCtx *m = static_cast<MultiCtx *>(mctx);
    if (!m || !model || !fh || !ks || !out_h || !fh->dev_off) return fail(HALDA_E_ARG, "NULL argument");
    const int nd = int(m->ctxs.size()), nf = fh->n_fleets;
    if (nf <= 0) return HALDA_OK;
    const int64_t xs = 7 * int64_t(std::max(fh->max_devices, 1)) + 1;
    std::vector<std::vector<int64_t>> offs(nd), xoffs(nd);
    std::vector<int> rcs(nd, HALDA_OK);
    std::vector<std::string> errs(nd);
    std::vector<std::thread> th;
    for (int r = 0; r < nd; ++r) {
        const int base = nf / nd, extra = nf % nd;
        const int lo = r * base + std::min(r, extra), hi = lo + base + (r < extra ? 1 : 0);
        if (hi <= lo) continue;
        const int64_t d0 = fh->dev_off[lo];
        offs[r].resize(size_t(hi - lo + 1));
        for (int f = lo; f <= hi; ++f) offs[r][size_t(f - lo)] = fh->dev_off[f] - d0;
        th.emplace_back([&, r, lo, hi, d0]() {
            halda_fleets sub = stage::shifted(*fh, d0);  // min / max devices stay the call's (valid for the block)
            sub.n_fleets = hi - lo;
            sub.dev_off = offs[r].data();
            halda_fleet_result o = *out_h;
            o.best_k = out_h->best_k + lo;
            o.obj_value = out_h->obj_value + lo;
            o.w = out_h->w + d0;
            o.n = out_h->n + d0;
            o.obj_by_k = out_h->obj_by_k ? out_h->obj_by_k + int64_t(lo) * n_k : nullptr;
            o.status = out_h->status ? out_h->status + int64_t(lo) * n_k : nullptr;
            if (out_h->x_off) {  // compact layout: the block's offsets relative to its first slot
                int64_t b0 = INT64_MAX;
                for (int64_t i = int64_t(lo) * n_k; i < int64_t(hi) * n_k; ++i)
                    if (out_h->x_off[i] >= 0) b0 = std::min(b0, out_h->x_off[i]);
                if (b0 == INT64_MAX) b0 = 0;
                xoffs[r].resize(size_t(hi - lo) * size_t(n_k));
                for (int64_t i = int64_t(lo) * n_k; i < int64_t(hi) * n_k; ++i)
                    xoffs[r][size_t(i - int64_t(lo) * n_k)] = out_h->x_off[i] >= 0 ? out_h->x_off[i] - b0 : -1;
                o.x_off = xoffs[r].data();
                o.x = out_h->x ? out_h->x + b0 : nullptr;
                o.c = out_h->c ? out_h->c + b0 : nullptr;
            } else {
                o.x = out_h->x ? out_h->x + int64_t(lo) * n_k * xs : nullptr;
                o.c = out_h->c ? out_h->c + int64_t(lo) * n_k * xs : nullptr;
            }
            rcs[r] = halda_solve_fleets_host(m->ctxs[size_t(r)], model, &sub, ks, n_k, &o);
            if (rcs[r] != HALDA_OK) errs[r] = g_err;
        });
    }
    for (auto &t : th) t.join();
    for (int r = 0; r < nd; ++r)
        if (rcs[r] != HALDA_OK) return fail(rcs[r], "device " + std::to_string(r) + ": " + errs[r]);
    return HALDA_OK;
}

int halda_comm_unique_id(void *id128) {
    if (!id128) return fail(HALDA_E_ARG, "NULL id");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    return HALDA_OK;
}

int halda_comm_init(void **comm, int world, int rank, const void *id128, int device_ordinal) {
    if (!comm || !id128 || world < 1 || rank < 0 || rank >= world) return fail(HALDA_E_ARG, "halda_comm_init: bad arguments");
    HIP_TRY(hipSetDevice(device_ordinal));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    NCCL_TRY(ncclCommInitRank(&c, world, id, rank));
    *comm = c;
    return HALDA_OK;
}

void halda_comm_destroy(void *comm) {
    if (comm) (void)ncclCommDestroy(static_cast<ncclComm_t>(comm));
}

int halda_solve_fleets_sharded(void *ctx, void *comm, const halda_model *model, const halda_fleets *fleets,
                               const int32_t *ks, int32_t n_k, halda_fleet_result *out, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !comm || !model || !fleets || !ks || !out) return fail(HALDA_E_ARG, "NULL argument");
    ncclComm_t cm = static_cast<ncclComm_t>(comm);
    int world = 0, rank = 0;
    NCCL_TRY(ncclCommCount(cm, &world));
    NCCL_TRY(ncclCommUserRank(cm, &rank));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    std::vector<ShardRank> R(1);
    R[0].rank = rank;
    R[0].o = *out;
    // the ranks' all-reduces over RCCL, on this rank's results, in the step order of shard_steps
    auto ar = [&](ShardField fld, size_t count) -> int {
        const halda_fleet_result &o = R[0].o;
        switch (fld) {
            case kShObj: NCCL_TRY(ncclAllReduce(o.obj_value, o.obj_value, count, ncclFloat64, ncclMin, cm, s)); break;
            case kShBestK: NCCL_TRY(ncclAllReduce(o.best_k, o.best_k, count, ncclInt32, ncclMin, cm, s)); break;
            case kShGroupStart: NCCL_TRY(ncclGroupStart()); break;
            case kShW: NCCL_TRY(ncclAllReduce(o.w, o.w, count, ncclInt32, ncclSum, cm, s)); break;
            case kShN: NCCL_TRY(ncclAllReduce(o.n, o.n, count, ncclInt32, ncclSum, cm, s)); break;
            case kShObk: NCCL_TRY(ncclAllReduce(o.obj_by_k, o.obj_by_k, count, ncclFloat64, ncclMin, cm, s)); break;
            case kShSt: NCCL_TRY(ncclAllReduce(o.status, o.status, count, ncclInt32, ncclMax, cm, s)); break;
            case kShGroupEnd: NCCL_TRY(ncclGroupEnd()); break;
        }
        return HALDA_OK;
    };
    return shard_steps(c, *model, *fleets, ks, n_k, world, R, s, ar);
}

int halda_solve_fleets_sharded_emulated(void *ctx, int32_t world, int32_t report_rank, const halda_model *model,
                                        const halda_fleets *fleets, const int32_t *ks, int32_t n_k,
                                        halda_fleet_result *out, void *stream) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !model || !fleets || !ks || !out) return fail(HALDA_E_ARG, "NULL argument");
    if (world < 1 || world > kEmuMaxWorld || report_rank < 0 || report_rank >= world)
        return fail(HALDA_E_ARG, "halda_solve_fleets_sharded_emulated: need 1 <= world <= 16, 0 <= report_rank < world");
    if (!out->best_k || !out->obj_value || !out->w || !out->n) return fail(HALDA_E_ARG, "halda_fleet_result: NULL");
    if (out->x || out->c) return fail(HALDA_E_ARG, "halda_solve_fleets_sharded: x / c are not gathered (pass NULL)");
    if (fleets->n_fleets > 0) {  // n_k, ks and the arrays before any size is computed or HIP call made
        const int rc = check_fleets_args(model, fleets, ks, n_k, out);
        if (rc != HALDA_OK) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const int64_t nf = fleets->n_fleets;
    if (nf <= 0) return HALDA_OK;
    int64_t nd = 0;
    {
        const int rc = shard_device_count(*fleets, s, &nd);
        if (rc != HALDA_OK) return rc;
    }
    // every virtual rank but report_rank gets its own result arrays (the caller's are report_rank's)
    stage::Bump lay;
    std::vector<stage::ResultSlots> slots;
    for (int r = 0; r < world; ++r) slots.push_back(stage::lay_result(lay, *out, nf, nd, size_t(nf) * n_k, 0));
    {
        const int rc = grow(&c->emu, &c->emu_bytes, lay.off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = static_cast<char *>(c->emu);
    std::vector<ShardRank> R(static_cast<size_t>(world));
    for (int r = 0; r < world; ++r) {
        R[size_t(r)].rank = r;
        halda_fleet_result &o = R[size_t(r)].o;
        if (r == report_rank) {
            o = *out;
            continue;
        }
        o = stage::bind_result(base, slots[size_t(r)], *out);  // x / c are NULL (checked above)
    }
    // each all-reduce as one device kernel over the virtual ranks' buffers (in place, every rank's copy
    // gets the reduced value), in the step order of shard_steps
    auto ar = [&](ShardField fld, size_t count) -> int {
        if (fld == kShGroupStart || fld == kShGroupEnd) return HALDA_OK;
        EmuReduce E = {};
        E.world = world;
        E.count = int64_t(count);
        E.field = int(fld);
        for (int r = 0; r < world; ++r) {
            const halda_fleet_result &o = R[size_t(r)].o;
            E.p[r] = fld == kShObj ? static_cast<void *>(o.obj_value) : fld == kShBestK ? static_cast<void *>(o.best_k)
                   : fld == kShW ? static_cast<void *>(o.w) : fld == kShN ? static_cast<void *>(o.n)
                   : fld == kShObk ? static_cast<void *>(o.obj_by_k) : static_cast<void *>(o.status);
        }
        if (count == 0) return HALDA_OK;
        hipLaunchKernelGGL(halda_emu_allreduce_kernel, dim3(unsigned((count + 255) / 256)), dim3(256), 0, s, E);
        HIP_TRY(hipGetLastError());
        return HALDA_OK;
    };
    return shard_steps(c, *model, *fleets, ks, n_k, world, R, s, ar);
}

int halda_last_lowered(void *ctx, halda_batch *lowered, halda_result *solved) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !lowered || !solved) return fail(HALDA_E_ARG, "NULL ctx/lowered/solved");
    if (!c->have_lowered)
        return fail(HALDA_E_ARG, "no lowered batch: the last halda_solve_fleets call ran the fused sweep "
                                 "(halda_set_fleets_path(ctx, 0) selects the CSR pipeline)");
    *lowered = c->last_lowered;
    *solved = c->last_solved;
    return HALDA_OK;
}

int halda_solve_batch(void *ctx, const halda_batch *in_h, halda_result *out_h) {
    Ctx *c = static_cast<Ctx *>(ctx);
    if (!c || !in_h || !out_h) return fail(HALDA_E_ARG, "NULL ctx/in/out");
    const halda_batch &h = *in_h;
    const int n = h.n_inst;
    if (n < 0) return fail(HALDA_E_ARG, "n_inst < 0");
    if (n == 0) return HALDA_OK;
    if (!h.n_cols || !h.n_rows || !h.csr_off || !h.col_off || !h.row_off || !h.row_ptr || !h.col_idx || !h.val ||
        !h.c || !h.col_lb || !h.col_ub || !h.row_lb || !h.row_ub || !h.integrality)
        return fail(HALDA_E_ARG, "halda_batch has a NULL array");
    if (!out_h->status || !out_h->x || !out_h->obj_lin || !out_h->dual_bound || !out_h->gap || !out_h->nodes)
        return fail(HALDA_E_ARG, "halda_result has a NULL array");
    int64_t n_colsum = 0, n_rowsum = 0, n_rp = 0, nnz = 0;
    halda_batch d = h;
    const bool need_summary = h.max_cols == 0 && h.max_R1 == 0 && h.max_tab == 0 && h.max_tab_kc == 0;
    if (need_summary) d.max_R1 = 1;
    for (int i = 0; i < n; ++i) {
        const int N = h.n_cols[i], m = h.n_rows[i];
        if (N < 1 || m < 1 || h.csr_off[i] < 0 || h.col_off[i] < 0 || h.row_off[i] < 0)
            return fail(HALDA_E_ARG, "instance " + std::to_string(i) + ": bad sizes/offsets");
        n_colsum = std::max<int64_t>(n_colsum, h.col_off[i] + N);
        n_rowsum = std::max<int64_t>(n_rowsum, h.row_off[i] + m);
        n_rp = std::max<int64_t>(n_rp, h.csr_off[i] + m + 1);
        nnz = std::max<int64_t>(nnz, int64_t(h.row_ptr[h.csr_off[i] + m]));
        if (need_summary) {
            d.max_cols = std::max(d.max_cols, N);
            if ((N - 1) % 7 == 0) {
                const int M = (N - 1) / 7;
                const double W = h.row_ub[h.row_off[i] + m - 1];
                double sum = 0.0;
                for (int j = 0; j < M; ++j) sum += std::ceil(h.col_lb[h.col_off[i] + j]);
                const double Rr = W - sum;
                if (Rr >= 0 && Rr < 1e6) {
                    const int R1 = int(Rr) + 1;
                    d.max_R1 = std::max(d.max_R1, R1);
                    if (h.c[h.col_off[i] + 7 * M] > 0) d.max_tab_kc = std::max(d.max_tab_kc, M * R1);
                    else d.max_tab = std::max(d.max_tab, M * R1);
                }
            }
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    stage::Bump lay;
    const size_t o_ncols = lay.take(4 * n), o_nrows = lay.take(4 * n), o_csr = lay.take(8 * n),
                 o_col = lay.take(8 * n), o_row = lay.take(8 * n), o_rp = lay.take(4 * n_rp),
                 o_ci = lay.take(4 * nnz), o_val = lay.take(8 * nnz), o_c = lay.take(8 * n_colsum), o_clb = lay.take(8 * n_colsum), o_cub = lay.take(8 * n_colsum),
                 o_rlb = lay.take(8 * n_rowsum), o_rub = lay.take(8 * n_rowsum), o_int = lay.take(n_colsum),
                 o_st = lay.take(4 * n), o_x = lay.take(8 * n_colsum), o_obj = lay.take(8 * n), o_db = lay.take(8 * n),
                 o_gap = lay.take(8 * n), o_nodes = lay.take(8 * n);
    {
        const int rc = ensure_scratch(c, lay.off);
        if (rc != HALDA_OK) return rc;
    }
    char *base = static_cast<char *>(c->scratch);
    hipStream_t s = c->stream;
    {
        const int rc = order_after_previous(c, s);
        if (rc != HALDA_OK) return rc;
    }
    auto up = [&](size_t o, const void *src, size_t bytes) {
        return hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, s);
    };
    HIP_TRY(up(o_ncols, h.n_cols, 4 * n));
    HIP_TRY(up(o_nrows, h.n_rows, 4 * n));
    HIP_TRY(up(o_csr, h.csr_off, 8 * n));
    HIP_TRY(up(o_col, h.col_off, 8 * n));
    HIP_TRY(up(o_row, h.row_off, 8 * n));
    HIP_TRY(up(o_rp, h.row_ptr, 4 * n_rp));
    HIP_TRY(up(o_ci, h.col_idx, 4 * nnz));
    HIP_TRY(up(o_val, h.val, 8 * nnz));
    HIP_TRY(up(o_c, h.c, 8 * n_colsum));
    HIP_TRY(up(o_clb, h.col_lb, 8 * n_colsum));
    HIP_TRY(up(o_cub, h.col_ub, 8 * n_colsum));
    HIP_TRY(up(o_rlb, h.row_lb, 8 * n_rowsum));
    HIP_TRY(up(o_rub, h.row_ub, 8 * n_rowsum));
    HIP_TRY(up(o_int, h.integrality, n_colsum));
    HIP_TRY(hipMemsetAsync(base + o_x, 0, 8 * n_colsum, s));
    d.n_cols = reinterpret_cast<const int32_t *>(base + o_ncols);
    d.n_rows = reinterpret_cast<const int32_t *>(base + o_nrows);
    d.csr_off = reinterpret_cast<const int64_t *>(base + o_csr);
    d.col_off = reinterpret_cast<const int64_t *>(base + o_col);
    d.row_off = reinterpret_cast<const int64_t *>(base + o_row);
    d.row_ptr = reinterpret_cast<const int32_t *>(base + o_rp);
    d.col_idx = reinterpret_cast<const int32_t *>(base + o_ci);
    d.val = reinterpret_cast<const double *>(base + o_val);
    d.c = reinterpret_cast<const double *>(base + o_c);
    d.col_lb = reinterpret_cast<const double *>(base + o_clb);
    d.col_ub = reinterpret_cast<const double *>(base + o_cub);
    d.row_lb = reinterpret_cast<const double *>(base + o_rlb);
    d.row_ub = reinterpret_cast<const double *>(base + o_rub);
    d.integrality = reinterpret_cast<const uint8_t *>(base + o_int);
    d.x0 = d.y0 = nullptr;
    halda_result r;
    r.status = reinterpret_cast<int32_t *>(base + o_st);
    r.x = reinterpret_cast<double *>(base + o_x);
    r.obj_lin = reinterpret_cast<double *>(base + o_obj);
    r.dual_bound = reinterpret_cast<double *>(base + o_db);
    r.gap = reinterpret_cast<double *>(base + o_gap);
    r.nodes = reinterpret_cast<int64_t *>(base + o_nodes);
    int rc = launch(c, d, r, s);
    if (rc != HALDA_OK) return rc;
    auto down = [&](void *dst, size_t o, size_t bytes) {
        return hipMemcpyAsync(dst, base + o, bytes, hipMemcpyDeviceToHost, s);
    };
    HIP_TRY(down(out_h->status, o_st, 4 * n));
    HIP_TRY(down(out_h->x, o_x, 8 * n_colsum));
    HIP_TRY(down(out_h->obj_lin, o_obj, 8 * n));
    HIP_TRY(down(out_h->dual_bound, o_db, 8 * n));
    HIP_TRY(down(out_h->gap, o_gap, 8 * n));
    HIP_TRY(down(out_h->nodes, o_nodes, 8 * n));
    HIP_TRY(hipStreamSynchronize(s));
    return HALDA_OK;
}

}  // extern "C"
