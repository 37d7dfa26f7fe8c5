// The host entry points' staging layer: where a call's table, inputs and results lie in the context's
// staging buffer, and the device-side structs that point there. Pure layout arithmetic on include/halda.h
// and the standard library -- no HIP call, so a host compiler builds it alone (tests/stage_layout.cpp);
// the copies themselves (ensure_scratch, upload, download) are in halda.hip next to grow().
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>

#include "halda.h"

namespace stage {

// Offsets handed out front to back, each region 256-byte aligned; `off` ends as the buffer's size.
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~size_t(255);
        return o;
    }
};

// The double arrays of a halda_fleets, in the order every layout and kernel argument uses.
constexpr int kFields = 16;
using Field = const double *halda_fleets::*;
constexpr Field kField[kFields] = {
    &halda_fleets::scpu_b1,     &halda_fleets::sgpu_b1,     &halda_fleets::T_cpu,         &halda_fleets::T_gpu,
    &halda_fleets::t_kvcpy_cpu, &halda_fleets::t_kvcpy_gpu, &halda_fleets::t_ram2vram,    &halda_fleets::t_vram2ram,
    &halda_fleets::t_comm,      &halda_fleets::s_disk,      &halda_fleets::d_avail_ram,   &halda_fleets::c_cpu,
    &halda_fleets::c_gpu,       &halda_fleets::d_avail_cuda, &halda_fleets::d_avail_metal, &halda_fleets::swap};

// No NULL array in the table.
inline bool complete(const halda_fleets &F) {
    bool ok = F.dev_off && F.os_class && F.flags;
    for (Field f : kField) ok = ok && F.*f;
    return ok;
}

// A table of nf fleets / nd devices in a staging buffer: dev_off, os_class, flags, then the fields as rows of
// one block of kFields x nd doubles (`split` < kFields: two blocks, the first of `split` rows --
// halda_solve_fleets_host's, whose total decides its transport).
struct TableLayout {
    int64_t nf, nd;
    size_t dev_off, os_class, flags, field[kFields];
};

inline TableLayout lay_table(Bump &b, int64_t nf, int64_t nd, int split = kFields) {
    TableLayout t{nf, nd, b.take(8 * (nf + 1)), b.take(nd), b.take(nd), {}};
    const size_t b0 = b.take(8 * nd * split), b1 = split < kFields ? b.take(8 * nd * (kFields - split)) : 0;
    for (int a = 0; a < kFields; ++a) t.field[a] = a < split ? b0 + 8 * nd * a : b1 + 8 * nd * (a - split);
    return t;
}

// F with its arrays at `base` + the layout's offsets (the scalar members copied).
inline halda_fleets rebase(const halda_fleets &F, const char *base, const TableLayout &t) {
    halda_fleets d = F;
    d.dev_off = reinterpret_cast<const int64_t *>(base + t.dev_off);
    d.os_class = reinterpret_cast<const uint8_t *>(base + t.os_class);
    d.flags = reinterpret_cast<const uint8_t *>(base + t.flags);
    for (int a = 0; a < kFields; ++a) d.*kField[a] = reinterpret_cast<const double *>(base + t.field[a]);
    return d;
}

// F with every per-device array moved on by d0 devices (dev_off is the caller's to set).
inline halda_fleets shifted(const halda_fleets &F, int64_t d0) {
    halda_fleets s = F;
    s.os_class += d0;
    s.flags += d0;
    for (Field f : kField) s.*f += d0;
    return s;
}

// The arrays of a halda_subfleets of n items / tot = sub_off[n] listed devices in a staging buffer.
struct ItemsLayout {
    int64_t n, tot;
    size_t parent, sub_off, sub_idx;
};

inline ItemsLayout lay_items(Bump &b, int64_t n, int64_t tot) {
    return {n, tot, b.take(4 * n), b.take(8 * (n + 1)), b.take(4 * tot)};
}

// I with its arrays at `base` + the layout's offsets (the scalar members copied).
inline halda_subfleets rebase(const halda_subfleets &I, const char *base, const ItemsLayout &t) {
    halda_subfleets d = I;
    d.parent = reinterpret_cast<const int32_t *>(base + t.parent);
    d.sub_off = reinterpret_cast<const int64_t *>(base + t.sub_off);
    d.sub_idx = reinterpret_cast<const int32_t *>(base + t.sub_idx);
    return d;
}

// The per-device int32 inputs of a frontier call -- w0, w_min, w_max, `count` entries each -- in a staging
// buffer: an array the host did not pass takes no room and stays NULL on the device.
struct TripleLayout {
    int64_t count;
    const int32_t *host[3];
    size_t off[3];
    const int32_t *at(const char *base, int a) const {
        return host[a] ? reinterpret_cast<const int32_t *>(base + off[a]) : nullptr;
    }
};

inline TripleLayout lay_triple(Bump &b, const int32_t *w0, const int32_t *w_min, const int32_t *w_max, int64_t count) {
    TripleLayout t{count, {w0, w_min, w_max}, {0, 0, 0}};
    for (int a = 0; a < 3; ++a) t.off[a] = t.host[a] ? b.take(4 * count) : 0;
    return t;
}

// Doubles that x (and c) hold. Row r has off[r + 1] - off[r] devices (dev_off, or the items' sub_off), and
// the slot of (repeat v, row r, k index j) is (v * n_rows + r) * n_k + j: n_repeat the variants (else 1),
// n_k = 1 for the plan evaluation's one slot per fleet. Without x_off the dense layout, stride
// 7 max_devices + 1 per slot; with it max(x_off + 7 M_r + 1) over the slots with x_off >= 0 (none: 0).
inline size_t xc_extent(const int64_t *off, int64_t n_rows, int64_t n_k, int64_t n_repeat, int64_t max_devices,
                        const int64_t *x_off) {
    if (!x_off) return size_t(n_repeat * n_rows * n_k) * (7 * size_t(std::max<int64_t>(max_devices, 1)) + 1);
    int64_t ext = 0;
    for (int64_t v = 0; v < n_repeat; ++v)
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t N = 7 * (off[r + 1] - off[r]) + 1;
            for (int64_t j = 0; j < n_k; ++j) {
                const int64_t a = x_off[(v * n_rows + r) * n_k + j];
                if (a >= 0) ext = std::max(ext, a + N);
            }
        }
    return size_t(ext);
}

// The compact x / c layout is in use: the caller passed x_off and wants x or c.
inline bool compact(const halda_fleet_result &h) { return h.x_off && (h.x || h.c); }

// A halda_fleet_result in a staging buffer, for the host's `h`: x_off (compact layout only), then best_k,
// obj_value, w, n, obj_by_k, status (always reserved), then x and c where the host passed them. rows: the
// fleets, items or variants x fleets; devs: their devices; n_inst: rows x n_k; ext: xc_extent.
struct ResultSlots {
    size_t rows, devs, n_inst, ext;
    size_t x_off, best_k, obj_value, w, n, obj_by_k, status, x, c;
};

inline ResultSlots lay_result(Bump &b, const halda_fleet_result &h, size_t rows, size_t devs, size_t n_inst,
                              size_t ext) {
    ResultSlots s{rows, devs, n_inst, ext, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    s.x_off = compact(h) ? b.take(8 * n_inst) : 0;
    s.best_k = b.take(4 * rows);
    s.obj_value = b.take(8 * rows);
    s.w = b.take(4 * devs);
    s.n = b.take(4 * devs);
    s.obj_by_k = b.take(8 * n_inst);
    s.status = b.take(4 * n_inst);
    s.x = h.x ? b.take(8 * ext) : 0;
    s.c = h.c ? b.take(8 * ext) : 0;
    return s;
}

// The device-side result at `base`: the optional arrays bound where the host passed them (per_k: obj_by_k and
// status whether or not it did -- halda_solve_fleets_host reads the statuses itself).
inline halda_fleet_result bind_result(char *base, const ResultSlots &s, const halda_fleet_result &h,
                                      bool per_k = false) {
    halda_fleet_result r;
    r.best_k = reinterpret_cast<int32_t *>(base + s.best_k);
    r.obj_value = reinterpret_cast<double *>(base + s.obj_value);
    r.w = reinterpret_cast<int32_t *>(base + s.w);
    r.n = reinterpret_cast<int32_t *>(base + s.n);
    r.obj_by_k = per_k || h.obj_by_k ? reinterpret_cast<double *>(base + s.obj_by_k) : nullptr;
    r.status = per_k || h.status ? reinterpret_cast<int32_t *>(base + s.status) : nullptr;
    r.x = h.x ? reinterpret_cast<double *>(base + s.x) : nullptr;
    r.c = h.c ? reinterpret_cast<double *>(base + s.c) : nullptr;
    r.x_off = compact(h) ? reinterpret_cast<const int64_t *>(base + s.x_off) : nullptr;
    return r;
}

// What comes back: (host pointer, offset, bytes); an entry with a NULL host pointer or no bytes is skipped.
struct Copy {
    void *host;
    size_t off, bytes;
};

inline std::array<Copy, 8> result_copies(const ResultSlots &s, const halda_fleet_result &h) {
    return {{{h.best_k, s.best_k, 4 * s.rows},
             {h.obj_value, s.obj_value, 8 * s.rows},
             {h.w, s.w, 4 * s.devs},
             {h.n, s.n, 4 * s.devs},
             {h.obj_by_k, s.obj_by_k, 8 * s.n_inst},
             {h.status, s.status, 4 * s.n_inst},
             {h.x, s.x, 8 * s.ext},
             {h.c, s.c, 8 * s.ext}}};
}

// A halda_frontier in a staging buffer: status, obj and moved per (fleet, point), then the w and n planes.
struct FrontierSlots {
    size_t pts, plane;  // n_fleets x (max_p + 1) points; (max_p + 1) x n_devices plane entries
    size_t status, obj, moved, w, n;
};

inline FrontierSlots lay_frontier(Bump &b, int64_t nf, int64_t nd, int64_t max_p) {
    FrontierSlots s{size_t(nf * (max_p + 1)), size_t(nd * (max_p + 1)), 0, 0, 0, 0, 0};
    s.status = b.take(4 * s.pts);
    s.obj = b.take(8 * s.pts);
    s.moved = b.take(4 * s.pts);
    s.w = b.take(4 * s.plane);
    s.n = b.take(4 * s.plane);
    return s;
}

inline halda_frontier bind_frontier(char *base, const FrontierSlots &s, int64_t nd) {
    halda_frontier r;
    r.n_devices = nd;
    r.status = reinterpret_cast<int32_t *>(base + s.status);
    r.obj = reinterpret_cast<double *>(base + s.obj);
    r.moved = reinterpret_cast<int32_t *>(base + s.moved);
    r.w = reinterpret_cast<int32_t *>(base + s.w);
    r.n = reinterpret_cast<int32_t *>(base + s.n);
    return r;
}

inline std::array<Copy, 5> frontier_copies(const FrontierSlots &s, const halda_frontier &h) {
    return {{{h.status, s.status, 4 * s.pts},
             {h.obj, s.obj, 8 * s.pts},
             {h.moved, s.moved, 4 * s.pts},
             {h.w, s.w, 4 * s.plane},
             {h.n, s.n, 4 * s.plane}}};
}

// The incumbents of a budget call: every w0_i >= 1 and every fleet's sum equal to W. -1, or the first fleet
// that breaks either.
inline int64_t bad_incumbent(const int64_t *dev_off, int64_t nf, const int32_t *w0, int64_t W) {
    for (int64_t f = 0; f < nf; ++f) {
        int64_t sum = 0;
        bool ok = true;
        for (int64_t i = dev_off[f]; i < dev_off[f + 1]; ++i) {
            ok = ok && w0[i] >= 1;
            sum += w0[i];
        }
        if (!ok || sum != W) return f;
    }
    return -1;
}

// A halda_change_frontier in a staging buffer: status, obj, loaded and released per (item, point), then the
// w and n planes over the listed devices.
struct ChangeSlots {
    size_t pts, plane;  // n_items x (max_p + 1) points; (max_p + 1) x sub_off[n_items] plane entries
    size_t status, obj, loaded, released, w, n;
};

inline ChangeSlots lay_change(Bump &b, int64_t n_items, int64_t tot, int64_t max_p) {
    ChangeSlots s{size_t(n_items * (max_p + 1)), size_t(tot * (max_p + 1)), 0, 0, 0, 0, 0, 0};
    s.status = b.take(4 * s.pts);
    s.obj = b.take(8 * s.pts);
    s.loaded = b.take(4 * s.pts);
    s.released = b.take(4 * s.pts);
    s.w = b.take(4 * s.plane);
    s.n = b.take(4 * s.plane);
    return s;
}

inline halda_change_frontier bind_change(char *base, const ChangeSlots &s, int64_t tot) {
    halda_change_frontier r;
    r.n_devices = tot;
    r.status = reinterpret_cast<int32_t *>(base + s.status);
    r.obj = reinterpret_cast<double *>(base + s.obj);
    r.loaded = reinterpret_cast<int32_t *>(base + s.loaded);
    r.released = reinterpret_cast<int32_t *>(base + s.released);
    r.w = reinterpret_cast<int32_t *>(base + s.w);
    r.n = reinterpret_cast<int32_t *>(base + s.n);
    return r;
}

inline std::array<Copy, 6> change_copies(const ChangeSlots &s, const halda_change_frontier &h) {
    return {{{h.status, s.status, 4 * s.pts},
             {h.obj, s.obj, 8 * s.pts},
             {h.loaded, s.loaded, 4 * s.pts},
             {h.released, s.released, 4 * s.pts},
             {h.w, s.w, 4 * s.plane},
             {h.n, s.n, 4 * s.plane}}};
}

// The incumbents of a change call, laid out by sub_off: every w0_i >= 0 and every item's deficit
// D = W - sum w0 in [0, max_deficit] (max_deficit < 0: no upper limit). Returns -1 and the largest deficit in
// *dmax, or the first item that breaks a rule.
inline int64_t bad_change(const int64_t *sub_off, int64_t n_items, const int32_t *w0, int64_t W, int64_t max_deficit,
                          int64_t *dmax) {
    int64_t top = 0;
    for (int64_t i = 0; i < n_items; ++i) {
        int64_t sum = 0;
        bool ok = true;
        for (int64_t j = sub_off[i]; j < sub_off[i + 1]; ++j) {
            ok = ok && w0[j] >= 0;
            sum += w0[j];
        }
        const int64_t D = W - sum;
        if (!ok || D < 0 || (max_deficit >= 0 && D > max_deficit)) return i;
        top = std::max(top, D);
    }
    *dmax = top;
    return -1;
}

// A halda_change_subset_frontier in a staging buffer: the five per-cell arrays over pts = n_fleets x D1 x
// (max_p + 1) cells, then the w and n plans of 64 entries per cell.
struct ChangeSubsetSlots {
    size_t pts;
    size_t status, obj, dropped_mask, loaded, released, w, n;
};

inline ChangeSubsetSlots lay_change_subsets(Bump &b, size_t pts) {
    ChangeSubsetSlots s{pts, 0, 0, 0, 0, 0, 0, 0};
    s.status = b.take(4 * pts);
    s.obj = b.take(8 * pts);
    s.dropped_mask = b.take(8 * pts);
    s.loaded = b.take(4 * pts);
    s.released = b.take(4 * pts);
    s.w = b.take(4 * 64 * pts);
    s.n = b.take(4 * 64 * pts);
    return s;
}

inline halda_change_subset_frontier bind_change_subsets(char *base, const ChangeSubsetSlots &s) {
    halda_change_subset_frontier r;
    r.status = reinterpret_cast<int32_t *>(base + s.status);
    r.obj = reinterpret_cast<double *>(base + s.obj);
    r.dropped_mask = reinterpret_cast<uint64_t *>(base + s.dropped_mask);
    r.loaded = reinterpret_cast<int32_t *>(base + s.loaded);
    r.released = reinterpret_cast<int32_t *>(base + s.released);
    r.w = reinterpret_cast<int32_t *>(base + s.w);
    r.n = reinterpret_cast<int32_t *>(base + s.n);
    return r;
}

inline std::array<Copy, 7> change_subsets_copies(const ChangeSubsetSlots &s, const halda_change_subset_frontier &h) {
    return {{{h.status, s.status, 4 * s.pts},
             {h.obj, s.obj, 8 * s.pts},
             {h.dropped_mask, s.dropped_mask, 8 * s.pts},
             {h.loaded, s.loaded, 4 * s.pts},
             {h.released, s.released, 4 * s.pts},
             {h.w, s.w, 4 * 64 * s.pts},
             {h.n, s.n, 4 * 64 * s.pts}}};
}

}  // namespace stage
