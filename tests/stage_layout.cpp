// The staging layer's layout arithmetic (distilp_amd/csrc/halda_stage.hpp, its pure part) checked on the
// CPU: built by tests/test_stage_layout.py with the host compiler and -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "halda_stage.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                     \
        }                                                                 \
    } while (0)

static size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// A table of the given fleet sizes: layout, rebasing, shifting, result slots.
static void check_table(const std::vector<int64_t> &sizes, int64_t n_k, int split) {
    const int64_t nf = int64_t(sizes.size());
    std::vector<int64_t> dev_off(1, 0);
    for (int64_t m : sizes) dev_off.push_back(dev_off.back() + m);
    const int64_t nd = dev_off.back();

    stage::Bump b;
    b.take(1);  // not at the buffer's start
    const size_t start = b.off;
    const stage::TableLayout t = stage::lay_table(b, nf, nd, split);
    // regions in order, 256-aligned, disjoint, the total the sum of the rounded sizes
    std::vector<size_t> at = {t.dev_off, t.os_class, t.flags, t.field[0]};
    std::vector<size_t> len = {size_t(8 * (nf + 1)), size_t(nd), size_t(nd), size_t(8 * nd * split)};
    if (split < stage::kFields) {
        at.push_back(t.field[split]);
        len.push_back(size_t(8 * nd * (stage::kFields - split)));
    }
    size_t want = start;
    for (size_t i = 0; i < at.size(); ++i) {
        CHECK(at[i] % 256 == 0);
        CHECK(at[i] == want);
        want += up256(len[i]);
    }
    CHECK(b.off == want);
    // the fields: rows of nd doubles within their block, in the canonical order
    for (int a = 0; a < stage::kFields; ++a) {
        const int first = a < split ? 0 : split;
        CHECK(t.field[a] == t.field[first] + size_t(8 * nd * (a - first)));
    }
    CHECK(t.nf == nf && t.nd == nd);

    // a host table with every array distinct; complete() sees each missing one
    std::vector<std::vector<double>> cols(stage::kFields, std::vector<double>(size_t(nd), 0.0));
    const size_t n_dev = size_t(nd);
    std::vector<uint8_t> cls(n_dev), flags(n_dev);
    halda_fleets F = {};
    F.n_fleets = int32_t(nf);
    F.min_devices = 1;
    F.max_devices = 5;
    F.dev_off = dev_off.data();
    F.os_class = cls.data();
    F.flags = flags.data();
    for (int a = 0; a < stage::kFields; ++a) F.*stage::kField[a] = cols[size_t(a)].data();
    CHECK(stage::complete(F));
    for (int a = 0; a < stage::kFields; ++a) {
        halda_fleets G = F;
        G.*stage::kField[a] = nullptr;
        CHECK(!stage::complete(G));
    }
    {
        halda_fleets G = F;
        G.flags = nullptr;
        CHECK(!stage::complete(G));
    }
    // the canonical order is the struct's own: consecutive pointer members from scpu_b1 to swap
    CHECK(F.scpu_b1 == cols[0].data() && F.s_disk == cols[9].data() && F.d_avail_ram == cols[10].data() &&
          F.d_avail_metal == cols[14].data() && F.swap == cols[15].data());

    // rebased: 16 + 3 pointers at the layout's offsets, scalars copied
    std::vector<char> buf(b.off);
    const halda_fleets d = stage::rebase(F, buf.data(), t);
    CHECK(d.n_fleets == F.n_fleets && d.min_devices == F.min_devices && d.max_devices == F.max_devices);
    CHECK(reinterpret_cast<const char *>(d.dev_off) == buf.data() + t.dev_off);
    CHECK(reinterpret_cast<const char *>(d.os_class) == buf.data() + t.os_class);
    CHECK(reinterpret_cast<const char *>(d.flags) == buf.data() + t.flags);
    for (int a = 0; a < stage::kFields; ++a)
        CHECK(reinterpret_cast<const char *>(d.*stage::kField[a]) == buf.data() + t.field[a]);

    // shifted by d0 devices: every per-device pointer moves by d0 elements, dev_off and the scalars stay
    const int64_t d0 = dev_off[size_t(nf) - 1];
    const halda_fleets s = stage::shifted(F, d0);
    CHECK(s.dev_off == F.dev_off && s.n_fleets == F.n_fleets && s.max_devices == F.max_devices);
    CHECK(s.os_class == F.os_class + d0 && s.flags == F.flags + d0);
    for (int a = 0; a < stage::kFields; ++a) CHECK(s.*stage::kField[a] == F.*stage::kField[a] + d0);

    // result slots: which regions exist follows the host's pointers; in order, aligned, disjoint
    const size_t n_inst = size_t(nf * n_k), ext = n_inst * 36 + 1;
    std::vector<int32_t> i32(1);
    std::vector<double> f64(1);
    std::vector<int64_t> i64(1);
    for (int mode = 0; mode < 3; ++mode) {  // 0: mandatory arrays only, 1: everything dense, 2: compact
        halda_fleet_result h = {};
        h.best_k = h.w = h.n = i32.data();
        h.obj_value = f64.data();
        if (mode >= 1) {
            h.obj_by_k = h.x = h.c = f64.data();
            h.status = i32.data();
        }
        if (mode == 2) h.x_off = i64.data();
        CHECK(stage::compact(h) == (mode == 2));
        stage::Bump rb;
        rb.take(300);
        size_t next = rb.off;
        const stage::ResultSlots R = stage::lay_result(rb, h, size_t(nf), size_t(nd), n_inst, ext);
        auto region = [&](size_t o, size_t bytes) {
            CHECK(o % 256 == 0);
            CHECK(o == next);
            next += up256(bytes);
        };
        if (mode == 2) region(R.x_off, 8 * n_inst);
        region(R.best_k, size_t(4 * nf));
        region(R.obj_value, size_t(8 * nf));
        region(R.w, size_t(4 * nd));
        region(R.n, size_t(4 * nd));
        region(R.obj_by_k, 8 * n_inst);  // reserved whether or not the host asked
        region(R.status, 4 * n_inst);
        if (mode >= 1) region(R.x, 8 * ext);
        if (mode >= 1) region(R.c, 8 * ext);
        CHECK(rb.off == next);
        std::vector<char> rbuf(rb.off);
        for (int per_k = 0; per_k < 2; ++per_k) {
            const halda_fleet_result r = stage::bind_result(rbuf.data(), R, h, per_k != 0);
            CHECK(reinterpret_cast<char *>(r.best_k) == rbuf.data() + R.best_k);
            CHECK(reinterpret_cast<char *>(r.obj_value) == rbuf.data() + R.obj_value);
            CHECK(reinterpret_cast<char *>(r.w) == rbuf.data() + R.w && reinterpret_cast<char *>(r.n) == rbuf.data() + R.n);
            const bool pk = per_k || mode >= 1;
            CHECK(reinterpret_cast<char *>(r.obj_by_k) == (pk ? rbuf.data() + R.obj_by_k : nullptr));
            CHECK(reinterpret_cast<char *>(r.status) == (pk ? rbuf.data() + R.status : nullptr));
            CHECK(reinterpret_cast<char *>(r.x) == (mode >= 1 ? rbuf.data() + R.x : nullptr));
            CHECK(reinterpret_cast<char *>(r.c) == (mode >= 1 ? rbuf.data() + R.c : nullptr));
            CHECK(reinterpret_cast<const char *>(r.x_off) == (mode == 2 ? rbuf.data() + R.x_off : nullptr));
        }
        const auto copies = stage::result_copies(R, h);
        const size_t bytes[8] = {size_t(4 * nf), size_t(8 * nf), size_t(4 * nd), size_t(4 * nd), 8 * n_inst,
                                 4 * n_inst,     8 * ext,        8 * ext};
        const void *host[8] = {h.best_k, h.obj_value, h.w, h.n, h.obj_by_k, h.status, h.x, h.c};
        const size_t offs[8] = {R.best_k, R.obj_value, R.w, R.n, R.obj_by_k, R.status, R.x, R.c};
        for (int a = 0; a < 8; ++a)
            CHECK(copies[size_t(a)].host == host[a] && copies[size_t(a)].bytes == bytes[a] &&
                  copies[size_t(a)].off == offs[a]);
    }
}

// The x / c extent: dense formula, compact maximum, all -1 -> 0, in the three indexings.
static void check_extent(const std::vector<int64_t> &sizes, int64_t n_k, int64_t n_rep) {
    const int64_t nf = int64_t(sizes.size());
    std::vector<int64_t> off(1, 0);
    int64_t mmax = 0;
    for (int64_t m : sizes) {
        off.push_back(off.back() + m);
        mmax = std::max(mmax, m);
    }
    const size_t slots = size_t(n_rep * nf * n_k);
    CHECK(stage::xc_extent(off.data(), nf, n_k, n_rep, mmax, nullptr) == slots * size_t(7 * mmax + 1));
    CHECK(stage::xc_extent(off.data(), nf, n_k, n_rep, 0, nullptr) == slots * 8);  // max_devices < 1 counts as 1
    std::vector<int64_t> x_off(slots, -1);
    CHECK(stage::xc_extent(off.data(), nf, n_k, n_rep, mmax, x_off.data()) == 0);
    // one slot at a time, far out: the extent is that slot's offset + 7 M_f + 1 whatever the others hold
    for (int64_t v = 0; v < n_rep; ++v)
        for (int64_t f = 0; f < nf; ++f)
            for (int64_t j = 0; j < n_k; ++j) {
                std::vector<int64_t> xo(slots, -1);
                for (size_t i = 0; i < slots; i += 2) xo[i] = int64_t(3 * i);  // small offsets elsewhere
                const size_t at = size_t((v * nf + f) * n_k + j);
                xo[at] = 100000 + int64_t(at);
                CHECK(stage::xc_extent(off.data(), nf, n_k, n_rep, mmax, xo.data()) ==
                      size_t(xo[at] + 7 * sizes[size_t(f)] + 1));
            }
}

// The items of the given list lengths: regions in order, 256-aligned, the total the sum of the rounded sizes;
// rebasing keeps the scalar members.
static void check_items(const std::vector<int64_t> &lens) {
    const int64_t n = int64_t(lens.size());
    int64_t tot = 0;
    for (int64_t m : lens) tot += m;
    stage::Bump b;
    b.take(1);
    const size_t start = b.off;
    const stage::ItemsLayout t = stage::lay_items(b, n, tot);
    CHECK(t.n == n && t.tot == tot);
    CHECK(t.parent == start && t.sub_off == t.parent + up256(size_t(4 * n)));
    CHECK(t.sub_idx == t.sub_off + up256(size_t(8 * (n + 1))) && b.off == t.sub_idx + up256(size_t(4 * tot)));
    halda_subfleets I = {};
    I.n_items = n;
    I.min_devices = 1;
    I.max_devices = 5;
    std::vector<char> buf(b.off);
    const halda_subfleets d = stage::rebase(I, buf.data(), t);
    CHECK(d.n_items == n && d.min_devices == 1 && d.max_devices == 5);
    CHECK(reinterpret_cast<const char *>(d.parent) == buf.data() + t.parent);
    CHECK(reinterpret_cast<const char *>(d.sub_off) == buf.data() + t.sub_off);
    CHECK(reinterpret_cast<const char *>(d.sub_idx) == buf.data() + t.sub_idx);
}

// w0 / w_min / w_max of `count` entries, each subset of them passed: an array that is not passed takes no
// room and stays NULL; the others lie in order, 256-aligned.
static void check_triple(int64_t count) {
    std::vector<int32_t> a(size_t(count), 0);
    for (int mask = 0; mask < 8; ++mask) {
        const int32_t *src[3];
        for (int i = 0; i < 3; ++i) src[i] = mask >> i & 1 ? a.data() : nullptr;
        stage::Bump b;
        b.take(1);
        size_t want = b.off;
        const stage::TripleLayout t = stage::lay_triple(b, src[0], src[1], src[2], count);
        std::vector<char> buf(b.off);
        CHECK(t.count == count);
        for (int i = 0; i < 3; ++i) {
            CHECK(t.host[i] == src[i]);
            if (!src[i]) {
                CHECK(t.at(buf.data(), i) == nullptr);
                continue;
            }
            CHECK(t.off[i] == want && reinterpret_cast<const char *>(t.at(buf.data(), i)) == buf.data() + want);
            want += up256(size_t(4 * count));
        }
        CHECK(b.off == want);
    }
}

int main() {
    const std::vector<int64_t> ragged = {2, 3, 5}, one = {1};
    for (const auto &lens : {ragged, one}) check_items(lens);
    for (int64_t count : {1, 10, 64, 65}) check_triple(count);
    for (const auto &sizes : {ragged, one})
        for (int split : {stage::kFields, 10}) check_table(sizes, 3, split);
    for (const auto &sizes : {ragged, one}) {
        check_extent(sizes, 3, 1);  // plain: (fleet, k)
        check_extent(sizes, 3, 2);  // variant-major: (variant, fleet, k)
        check_extent(sizes, 1, 1);  // one slot per fleet (the plan evaluation)
    }
    // the bump allocator itself
    stage::Bump b;
    CHECK(b.take(0) == 0 && b.off == 0);
    CHECK(b.take(1) == 0 && b.off == 256);
    CHECK(b.take(256) == 256 && b.off == 512);
    CHECK(b.take(257) == 512 && b.off == 1024);
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("stage layout ok\n");
    return 0;
}
