// libhalda host side: what a context remembers of its last fused-sweep launch, the entry families' path /
// route knobs, and the i-th slice of a variant- or box-major result. No HIP: halda.hip includes it, and
// tests/launch_record.cpp builds it alone with the host compiler.
#pragma once

#include <cstdint>

#include "halda.h"

namespace lrec {

// ---- the launch record: which kernels the context's last halda_solve_fleets-like call enqueued
enum class Record {
    none,                     // nothing yet
    csr,                      // the CSR pipeline (lowering .. pick: halda_last_fleet_ms slots 2 .. 6)
    reg_alone,                // the register kernel (or a family's kernel under its gate) alone
    tables_alone,             // the table kernel (or a family's table kernel) alone
    reg_then_tables,          // the register launch, then the gated table (or global-table) launch
    seg_then_tables,          // the segment launch, then the gated table launch
    kslot_then_tables,        // the k-slot launch, then the gated table launch
    steps_alone,              // a group's steps launch
    kslot_steps_then_tables,  // a group's k-slot steps launch, then its gated table launch
};

// halda_last_fleet_ms's slots of a fused record: evf0 .. evf1 in `first` when second < 0, else evf0 .. evfm in
// `first` and evfm .. evf1 in `second`. first < 0: not a fused record (none, csr).
struct Slots {
    int first, second;
};

constexpr Slots record_slots(Record r) {
    switch (r) {
        case Record::reg_alone:
        case Record::steps_alone: return {0, -1};
        case Record::tables_alone: return {1, -1};
        case Record::reg_then_tables: return {0, 1};
        case Record::seg_then_tables: return {7, 1};
        case Record::kslot_then_tables:
        case Record::kslot_steps_then_tables: return {8, 1};
        default: return {-1, -1};
    }
}

// ---- the families' knobs: halda_set_<family>_path / halda_last_<family>_route
enum Family { kSubfleets, kSubsets, kVariants, kPlans, kBounds, kBoxes, kFamilies };

struct Knob {
    int path = 0;   // 0: automatic
    int route = 0;  // of the family's last call (0: none yet)
};

// a family's paths are 0 .. max_path; `message`: the setter's error text for any other
struct KnobRule {
    int max_path;
    const char *message;
};

constexpr KnobRule kKnobRules[kFamilies] = {
    {1, "sub-fleets path must be 0 (automatic) or 1 (always expand)"},
    {1, "subsets path must be 0 (automatic) or 1 (always expand)"},
    {1, "variants path must be 0 (automatic) or 1 (always loop)"},
    {2, "plans path must be 0 (automatic), 1 (always two launches) or 2 (fused where it applies)"},
    {3, "bounds path must be 0 (automatic), 1 (always general), 2 (fused where it applies) or "
        "3 (fused, else the table launch, where they apply)"},
    {1, "boxes path must be 0 (automatic) or 1 (always loop)"},
};

// nullptr when `path` is one of the family's, else the setter's message
constexpr const char *path_error(Family f, int path) {
    return path >= 0 && path <= kKnobRules[f].max_path ? nullptr : kKnobRules[f].message;
}

// A family's path forced for a nested call and put back on every way out; keep_route: the route too (the
// nested call is another family's entry and must not show in that family's answer).
class PathOverride {
  public:
    PathOverride(Knob &k, int path, bool keep_route = false) : k_(k), saved_(k), keep_route_(keep_route) {
        k.path = path;
    }
    ~PathOverride() {
        k_.path = saved_.path;
        if (keep_route_) k_.route = saved_.route;
    }
    PathOverride(const PathOverride &) = delete;
    PathOverride &operator=(const PathOverride &) = delete;

  private:
    Knob &k_;
    const Knob saved_;
    const bool keep_route_;
};

// ---- slice i of every output array of a result that holds one slice per variant / box: nf fleets and n_k
// k per slice; w and n advance by nd_at, the caller's i * (devices per slice)
inline halda_fleet_result result_slice(const halda_fleet_result &out, int64_t i, int64_t nf, int64_t nd_at,
                                       int64_t n_k, int64_t xstride) {
    halda_fleet_result o = out;
    o.best_k += i * nf;
    o.obj_value += i * nf;
    o.w += nd_at;
    o.n += nd_at;
    if (o.obj_by_k) o.obj_by_k += i * nf * n_k;
    if (o.status) o.status += i * nf * n_k;
    if (o.x_off) {
        o.x_off += i * nf * n_k;  // absolute offsets into the one x / c
    } else {
        if (o.x) o.x += i * nf * n_k * xstride;
        if (o.c) o.c += i * nf * n_k * xstride;
    }
    return o;
}

}  // namespace lrec
