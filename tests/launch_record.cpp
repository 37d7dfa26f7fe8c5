// The pure parts of libhalda's launch bookkeeping (distilp_amd/csrc/halda_launch.hpp) checked on the CPU:
// built by tests/test_launch_record.py with the host compiler and -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "halda_launch.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                     \
        }                                                                 \
    } while (0)

using lrec::Record;

// ---- 1: the record against the five booleans it replaced. Each row: the record, and what the host side wrote
// for that launch before (two launches, the register launch alone, segment first, k-slot first, fused at all).
struct Old {
    Record r;
    bool two, reg_alone, seg, kslot, fused;
};
static const Old kOld[] = {
    {Record::none, false, false, false, false, false},
    {Record::csr, false, false, false, false, false},
    {Record::reg_alone, false, true, false, false, true},               // kRegAlone and the families' register kernels
    {Record::tables_alone, false, false, false, false, true},           // kTablesAlone and the families' table kernels
    {Record::reg_then_tables, true, false, false, false, true},         // kRegGated, kRegBig
    {Record::seg_then_tables, true, false, true, false, true},          // kSegGated
    {Record::kslot_then_tables, true, false, false, true, true},        // kKslotGated
    {Record::steps_alone, false, true, false, false, true},             // the group launch, register form
    {Record::kslot_steps_then_tables, true, false, false, true, true},  // the group launch, k-slot form
};

// halda_last_fleet_ms's decoding of those booleans, as it stood: the slot of evf0 .. evfm (or evf0 .. evf1 for
// one launch) and of evfm .. evf1 (-1: one launch); {-1, -1}: not a fused record
static lrec::Slots old_slots(const Old &o) {
    if (!o.fused) return {-1, -1};
    if (o.two) return {o.kslot ? 8 : o.seg ? 7 : 0, 1};
    return {o.reg_alone ? 0 : 1, -1};
}

static void check_records() {
    CHECK(sizeof kOld / sizeof kOld[0] == size_t(Record::kslot_steps_then_tables) + 1);
    for (size_t i = 0; i < sizeof kOld / sizeof kOld[0]; ++i) {
        CHECK(size_t(kOld[i].r) == i);  // every value once, in the enum's order
        const lrec::Slots got = lrec::record_slots(kOld[i].r), want = old_slots(kOld[i]);
        CHECK(got.first == want.first && got.second == want.second);
        CHECK(got.first < 9 && got.second < 9);
    }
}

// ---- 2: the setters' ranges and messages, as each halda_set_<family>_path had them
struct OldRule {
    lrec::Family f;
    int lo, hi;
    const char *message;
};
static const OldRule kOldRules[] = {
    {lrec::kSubfleets, 0, 1, "sub-fleets path must be 0 (automatic) or 1 (always expand)"},
    {lrec::kSubsets, 0, 1, "subsets path must be 0 (automatic) or 1 (always expand)"},
    {lrec::kVariants, 0, 1, "variants path must be 0 (automatic) or 1 (always loop)"},
    {lrec::kPlans, 0, 2, "plans path must be 0 (automatic), 1 (always two launches) or 2 (fused where it applies)"},
    {lrec::kBounds, 0, 3,
     "bounds path must be 0 (automatic), 1 (always general), 2 (fused where it applies) or 3 (fused, else the table "
     "launch, where they apply)"},
    {lrec::kBoxes, 0, 1, "boxes path must be 0 (automatic) or 1 (always loop)"},
};

static void check_knobs() {
    CHECK(sizeof kOldRules / sizeof kOldRules[0] == size_t(lrec::kFamilies));
    const int probes[] = {-2147483647 - 1, -2, -1, 0, 1, 2, 3, 4, 5, 2147483647};
    for (const OldRule &r : kOldRules)
        for (int p : probes) {
            const char *why = lrec::path_error(r.f, p);
            if (p >= r.lo && p <= r.hi) CHECK(why == nullptr);
            else CHECK(why != nullptr && std::strcmp(why, r.message) == 0);
        }
    // the scoped override: the path back on the way out, the route only where asked
    lrec::Knob k;
    k.path = 2;
    k.route = 1;
    {
        const lrec::PathOverride o(k, 3);
        CHECK(k.path == 3 && k.route == 1);
        k.route = 2;  // the nested call's own answer
    }
    CHECK(k.path == 2 && k.route == 2);
    {
        const lrec::PathOverride o(k, 1, true);
        CHECK(k.path == 1);
        k.route = 3;
    }
    CHECK(k.path == 2 && k.route == 2);
}

// ---- 3: result_slice against the two loops it replaced (the variants loop: w / n move only for v != 0; the
// boxes loop: by `at`), as offsets from the arrays' starts
struct Arrays {
    std::vector<int32_t> best_k, w, n, status;
    std::vector<double> obj_value, obj_by_k, x, c;
    std::vector<int64_t> x_off;
};

static void check_slice(bool with_x_off, bool with_optional, int64_t i) {
    const int64_t nf = 3, nd = 7, n_k = 2, xstride = 15, slices = 3;
    Arrays A;
    A.best_k.resize(slices * nf);
    A.obj_value.resize(slices * nf);
    A.w.resize(slices * nd);
    A.n.resize(slices * nd);
    A.obj_by_k.resize(slices * nf * n_k);
    A.status.resize(slices * nf * n_k);
    A.x.resize(slices * nf * n_k * xstride);
    A.c.resize(slices * nf * n_k * xstride);
    A.x_off.resize(slices * nf * n_k);
    halda_fleet_result out = {};
    out.best_k = A.best_k.data();
    out.obj_value = A.obj_value.data();
    out.w = A.w.data();
    out.n = A.n.data();
    if (with_optional) {
        out.obj_by_k = A.obj_by_k.data();
        out.status = A.status.data();
        out.x = A.x.data();
        out.c = A.c.data();
    }
    if (with_x_off) out.x_off = A.x_off.data();
    // The callers' own offsets. The boxes loop: `at = b ? b * nd : 0` with nd read back whenever n_box > 1. The
    // variants loop: `v ? v * nd : 0`, where for a single variant nd was never read back and is -1 -- slice 0
    // must come out in place all the same.
    const int64_t nd_variants = i == 0 ? -1 : nd;  // what the variants loop holds at slice 0 of a one-variant call
    const int64_t at_variants = i ? i * nd_variants : 0, at_boxes = i ? i * nd : 0;
    for (int64_t at : {at_variants, at_boxes}) {
        const halda_fleet_result o = lrec::result_slice(out, i, nf, at, n_k, xstride);
        CHECK(o.best_k == out.best_k + i * nf && o.obj_value == out.obj_value + i * nf);
        CHECK(o.w == out.w + i * nd && o.n == out.n + i * nd);
        if (with_optional) {
            CHECK(o.obj_by_k == out.obj_by_k + i * nf * n_k && o.status == out.status + i * nf * n_k);
            // compact x / c: x_off holds absolute offsets, so x and c stay and x_off moves
            const int64_t xs = with_x_off ? 0 : i * nf * n_k * xstride;
            CHECK(o.x == out.x + xs && o.c == out.c + xs);
        } else {
            CHECK(!o.obj_by_k && !o.status && !o.x && !o.c);
        }
        if (with_x_off) CHECK(o.x_off == out.x_off + i * nf * n_k);
        else CHECK(!o.x_off);
    }
}

int main() {
    check_records();
    check_knobs();
    for (int x = 0; x < 2; ++x)
        for (int opt = 0; opt < 2; ++opt)
            for (int64_t i : {0, 2}) check_slice(x != 0, opt != 0, i);
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("launch record ok\n");
    return 0;
}
