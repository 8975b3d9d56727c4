// CPU check of speq_amd/csrc/build_limits.hpp (tests/test_build_limits_cpu.py compiles this with plain g++ and no ROCm
// include path: that it compiles is the proof that the header needs no HIP). Includes nothing of the project but that
// header. Every decision is checked on both sides of its edge, the edge worked out here by other arithmetic than the
// header's; then, over a sweep, what the kernels form from a layout is checked against the span it was laid out for.
// Prints "ok" and the figures the test reads, or the failed checks and exits 1.
#include "build_limits.hpp"

#include <cstdio>
#include <initializer_list>

namespace L = speq::limits;

static int g_failed = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: CHECK(%s) failed\n", __LINE__, #c);    \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

constexpr uint64_t SPAN = 1ull << 32;
constexpr uint32_t FILTER_BITS = 16, COVER = 12, BSLOTS = 4;  // ax_common.hpp, ax_scan.hip, scan_kernels.hip

// the smallest free_b whose usable nine tenths reach x: nine tenths are counted in whole tenths of free_b, so it is
// ten times the tenths needed
static uint64_t smallest_free_for(uint64_t x) { return (x + 8) / 9 * 10; }

static void free_memory_edges() {
    CHECK(L::usable(0) == 0 && L::usable(9) == 0 && L::usable(10) == 9 && L::usable(19) == 9 && L::usable(20) == 18);
    for (uint64_t n : {1ull, 95ull, 96000ull, 4194305ull, 200000000ull, (1ull << 30) - 1}) {
        const L::AxNeed a = L::ax_need(n);
        // the arrays alive before the table: gran, owner (n + 1 words), codes (n + 64), the counter (16), text2 + tbad
        CHECK(a.need >= a.gran_bytes + (n + 1) * 4 + (n + 64) + 16 + a.nw64 * 24);
        CHECK(a.gran_bytes == a.n_gran * 16 && a.n_gran * 32 >= n + 224);  // a run from any p < n reads 7 more granules
        CHECK(a.nw64 * 64 >= n + 256);
        const uint64_t f1 = smallest_free_for(a.need);
        for (uint64_t f = f1 - 12; f <= f1 + 12; ++f) {
            CHECK(L::ax_build_fits(a, f) == (f >= f1));
            CHECK(L::fits(a.need, f) == (f >= f1));
        }
        CHECK(L::ax_build_fits(a, a.need * 10 / 9) == (a.need * 10 / 9 >= f1));
        CHECK(!L::ax_build_fits(a, a.need));  // the bytes themselves are not enough: a tenth stays free
        // the sort: strictly more than n * 60 + need (the suffix array's 4 B per symbol are part of the 60)
        const uint64_t f2 = smallest_free_for(n * 60 + a.need + 1);
        for (uint64_t f = f2 - 12; f <= f2 + 12; ++f) CHECK(L::ax_sort_fits(n, a, f) == (f >= f2));
        CHECK(f2 > f1);  // (so the sort can be skipped while the build goes on)
        // the EM arrays: two of (n + 64) words
        CHECK(L::ax_em_bytes(n) == 2 * (n + 64) * 4);
        const uint64_t f3 = smallest_free_for(L::ax_em_bytes(n));
        for (uint64_t f = f3 - 12; f <= f3 + 12; ++f) CHECK(L::ax_em_fits(n, f) == (f >= f3));
    }
    CHECK(!L::ax_em_fits(96000, 0) && !L::ax_build_fits(L::ax_need(96000), 0) && !L::ax_sort_fits(1, L::ax_need(1), 0));
}

static uint64_t distinct_for_nb(uint64_t nb, uint32_t load) {  // the smallest distinct whose layout has nb buckets
    uint64_t lo = 0, hi = 1ull << 34;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (L::ax_layout(1, 21, mid, 1, load, FILTER_BITS, 0, false, 1ull << 40).nb >= nb) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

static void offset_edges() {
    // the comparison itself, at the real span: 2^32 - 64 is beyond, one less is not
    CHECK(L::ax_beyond(SPAN - 64, SPAN) && !L::ax_beyond(SPAN - 65, SPAN));
    CHECK(L::ax_beyond(1000 - 64, 1000) && !L::ax_beyond(1000 - 65, 1000));
    // buckets: nb * 64 = 2^32 - 64 at nb = 2^26 - 1
    for (uint32_t load : {10u, 35u, 90u}) {
        const uint64_t d_edge = distinct_for_nb((1ull << 26) - 1, load);
        const L::AxLayout at = L::ax_layout(d_edge, 21, d_edge, 4, load, FILTER_BITS, 0, true, SPAN);
        const L::AxLayout below = L::ax_layout(d_edge, 21, d_edge - 1, 4, load, FILTER_BITS, 0, true, SPAN);
        CHECK(at.refused && at.nb == 0 && at.atab_bytes == 0);
        CHECK(!below.refused && below.nb == (1ull << 26) - 2 && below.nb * 64 == SPAN - 128);
        CHECK(below.s_words == 0);  // (no room for a bitmap that close to the span)
        // the k-mer filter's own clause (nf * 8 = 2 distinct) is reached long after the buckets' (>= 8.8 distinct)
        CHECK(below.nf * 8 < SPAN / 4);
    }
    // the m-mer filter: dropped at nb * 64 + nmf * 8 + 16 = limit - 64, kept one below; the table is refused later
    for (uint64_t distinct : {1000ull, 90000ull, 3000000ull}) {
        const uint32_t k = 70, load = 35;
        const uint64_t n = distinct + 500, n_texts = 8;
        const uint32_t m = L::ax_mfilter_m(n, k, COVER);
        CHECK(m != 0);
        const L::AxLayout free_ = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, SPAN);
        CHECK(!free_.refused && free_.m == m && free_.nmf == (distinct + n_texts * k) * FILTER_BITS / 64);
        CHECK(free_.s_off == free_.nb * 64 + free_.nmf * 8 + 16 && free_.s_words == (n + 255) / 256 * 4);
        CHECK(free_.s_bytes == free_.s_words * 8 + 16 && free_.atab_bytes == free_.s_off + free_.s_bytes);
        // bitmap: the smallest limit that keeps it is its end + 64 + 1
        const uint64_t s_end = free_.s_off + free_.s_words * 8 + 16;
        const L::AxLayout s_keep = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, s_end + 65);
        const L::AxLayout s_drop = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, s_end + 64);
        CHECK(s_keep.s_words == free_.s_words && s_keep.atab_bytes == free_.atab_bytes);
        CHECK(!s_drop.refused && s_drop.s_words == 0 && s_drop.s_bytes == 0 && s_drop.m == m);
        CHECK(s_drop.atab_bytes == s_drop.s_off && s_drop.s_off == free_.s_off);
        // m-mer filter
        const uint64_t mf_end = free_.nb * 64 + free_.nmf * 8 + 16;
        const L::AxLayout m_keep = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, mf_end + 65);
        const L::AxLayout m_drop = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, mf_end + 64);
        CHECK(!m_keep.refused && m_keep.m == m && m_keep.nmf == free_.nmf && m_keep.s_words == 0);
        CHECK(!m_drop.refused && m_drop.m == 0 && m_drop.nmf == 0 && m_drop.nb == free_.nb);
        CHECK(m_drop.s_off == free_.nb * 64);  // the bitmap moves up behind the buckets ...
        CHECK((m_drop.s_words != 0) == (free_.nb * 64 + free_.s_words * 8 + 16 < mf_end));  // ... where it fits
        // buckets
        const L::AxLayout b_keep = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, free_.nb * 64 + 65);
        const L::AxLayout b_drop = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, free_.nb * 64 + 64);
        CHECK(!b_keep.refused && b_keep.m == 0 && b_keep.s_words == 0 && b_keep.atab_bytes == free_.nb * 64);
        CHECK(b_drop.refused);
        // k-mer filter: only below the buckets' own edge when the filter is the larger array, which it never is
        CHECK(free_.nf * 8 < free_.nb * 64);
    }
}

// what k_scan_ax and the builds form from a layout, in 64 bits, against the span the layout was made for
static void layout_is_addressable(const L::AxLayout& a, uint64_t limit, uint64_t* kept_m, uint64_t* kept_s) {
    if (a.refused) return;
    CHECK(a.nb >= 1 && a.nf >= 1);
    CHECK(a.nb * 64 < limit - 64 && a.nf * 8 < limit - 64);  // the last bucket's fourth 16-B load ends at nb * 64
    if (a.m) {
        CHECK(a.nmf >= 1);
        CHECK(a.nb * 64 + (a.nmf - 1) * 8 + 16 < limit - 64);  // a 16-B load of the last 8-B word
        ++*kept_m;
    } else {
        CHECK(a.nmf == 0);
    }
    CHECK(a.s_off == a.nb * 64 + (a.m ? a.nmf * 8 + 16 : 0));
    if (a.s_words) {
        CHECK(a.s_off + (a.s_words - 1) * 8 + 16 < limit - 64);
        ++*kept_s;
    }
    CHECK(a.atab_bytes == a.s_off + a.s_bytes && a.atab_bytes < limit);
    CHECK((uint64_t)(uint32_t)a.s_off == a.s_off && (uint64_t)(uint32_t)(a.nb * 64) == a.nb * 64);
    for (bool sp : {false, true})
        for (bool mf : {false, true}) {
            const uint64_t len = L::ax_atab_desc_len(a, sp, mf);
            const uint64_t exact = sp && a.s_words ? a.s_off + a.s_bytes : a.nb * 64 + (mf && a.m ? a.nmf * 8 + 16 : 0);
            CHECK(len == exact && len <= a.atab_bytes);
            CHECK(len <= 0xFFFFFFF0ull);  // the offset of a lane with nothing to load stays out of range
        }
}

static void sweep(uint64_t* n_layouts) {
    uint64_t kept_m = 0, kept_s = 0, dropped_m_only = 0, refused = 0, dropped_s_only = 0;
    for (uint64_t n : {1ull, 300ull, 96200ull, 4200000ull, 200000000ull, (1ull << 30) - 1})
        for (uint32_t k : {1u, 21u, 31u, 32u, 33u, 70u, 128u})
            for (uint64_t dpc : {0ull, 1ull, 50ull, 100ull})  // distinct k-mers, percent of n
                for (uint64_t n_texts : {1ull, 8ull, 40000ull})
                    for (uint32_t load : {10u, 35u, 90u}) {
                        const uint64_t distinct = n * dpc / 100;
                        const uint32_t m = L::ax_mfilter_m(n, k, COVER);
                        CHECK(m == 0 || (m >= 12 && m <= 32 && k + 1 >= m + COVER));
                        const L::AxLayout full = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, 1ull << 40);
                        const uint64_t ends[4] = {full.nb * 64, full.nb * 64 + full.nmf * 8 + 16,
                                                  full.s_off + full.s_words * 8 + 16, full.nf * 8};
                        uint64_t limits[13] = {SPAN};
                        int nl = 1;
                        for (uint64_t e : ends)
                            for (uint64_t d : {63ull, 64ull, 65ull}) limits[nl++] = e + d;
                        for (int i = 0; i < nl; ++i) {
                            const uint64_t limit = limits[i];
                            if (limit > SPAN || limit < 4096) continue;
                            const L::AxLayout a = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, m, true, limit);
                            layout_is_addressable(a, limit, &kept_m, &kept_s);
                            ++*n_layouts;
                            // the filter is given up before the table: refused only when the bare buckets, or the
                            // k-mer filter, are beyond the limit
                            const L::AxLayout bare = L::ax_layout(n, k, distinct, n_texts, load, FILTER_BITS, 0, false, limit);
                            CHECK(a.refused == bare.refused);
                            CHECK(a.refused == (full.nb * 64 >= limit - 64 || full.nf * 8 >= limit - 64));
                            if (a.refused) ++refused;
                            else if (m && !a.m) ++dropped_m_only;
                            else if (!a.s_words) ++dropped_s_only;
                            // the third free-memory check covers exactly what is allocated after it
                            if (!a.refused) {
                                const uint64_t bytes = a.atab_bytes + a.nf * 8;
                                CHECK(L::ax_table_fits(a, smallest_free_for(bytes)));
                                CHECK(!L::ax_table_fits(a, smallest_free_for(bytes) - 1));
                            }
                        }
                    }
    CHECK(kept_m > 0 && kept_s > 0 && dropped_m_only > 0 && dropped_s_only > 0 && refused > 0);
}

static void plane_edges() {
    // three-symbol planes: 64 * nb * 16 wraps at nb = 2^22; two-symbol planes: 16 * nb * 16 at nb = 2^24
    const struct {
        uint64_t planes, last_ok;
    } fam[] = {{64, 4194303}, {16, 16777215}};
    for (const auto& f : fam) {
        CHECK(L::planes_addressable(f.planes, f.last_ok, SPAN));
        CHECK(!L::planes_addressable(f.planes, f.last_ok + 1, SPAN));
        for (uint64_t nb : {f.last_ok, f.last_ok + 1}) {
            // what the device forms in 32 bits (scan_device.hpp): the family's size and the last entry's offset
            const uint32_t nb32 = (uint32_t)nb;
            const uint32_t size32 = (uint32_t)f.planes * nb32 * 16u;
            const uint32_t last32 = ((uint32_t)f.planes - 1u) * nb32 * 16u + (nb32 - 1u) * 16u;
            const uint64_t size64 = f.planes * nb * 16, last64 = (f.planes - 1) * nb * 16 + (nb - 1) * 16;
            const bool exact = size32 == size64 && last32 == last64 && size64 <= 0xFFFFFFF0ull;
            CHECK(exact == L::planes_addressable(f.planes, nb, SPAN));
        }
    }
    // by symbols: an index of n symbols has n / 96 + 1 blocks, so 2^22 of them from n = 402,653,088 and 2^24 from
    // n = 1,610,612,640
    CHECK(L::plane_families(402653087 / 96 + 1, true, true, SPAN).occ3);
    CHECK(!L::plane_families(402653088 / 96 + 1, true, true, SPAN).occ3);
    CHECK(L::plane_families(402653088 / 96 + 1, true, true, SPAN).occ2);
    CHECK(L::plane_families(1610612639 / 96 + 1, true, true, SPAN).occ2);
    CHECK(!L::plane_families(1610612640 / 96 + 1, true, true, SPAN).occ2);
    CHECK(L::plane_families(((1ull << 31) - 1) / 96 + 1, true, true, SPAN).occ);  // every index fm_build accepts
    // what the file lacks is never published, and the three-symbol planes need the two-symbol ones
    for (uint64_t nb : {1ull, 1001ull, 4194303ull, 4194304ull, 16777216ull, 22369622ull})
        for (int has2 = 0; has2 < 2; ++has2)
            for (int has3 = 0; has3 < 2; ++has3)
                for (uint64_t limit : {SPAN, 64 * nb * 16 + 16, 64 * nb * 16 + 15, 16 * nb * 16 + 16, 16 * nb * 16 + 15}) {
                    if (limit > SPAN) continue;
                    const L::PlaneFamilies p = L::plane_families(nb, has2 != 0, has3 != 0, limit);
                    CHECK(p.occ2 == (has2 && 16 * nb * 16 + 16 <= limit));
                    CHECK(p.occ3 == (has2 && has3 && 64 * nb * 16 + 16 <= limit));
                    CHECK(!p.occ3 || p.occ2);
                    CHECK(p.occ == (5 * nb * 16 + 16 <= limit));
                }
}

static void ktab_edges(uint64_t* compact_fired_default) {
    CHECK(L::next_pow2(0) == 1 && L::next_pow2(1) == 1 && L::next_pow2(3) == 4 && L::next_pow2(4) == 4);
    for (uint64_t total : {0ull, 1ull, 17ull, 31ull, 32ull, 33ull, 95000ull, 131072ull, 4000000ull, 1ull << 31})
        for (uint64_t n_texts : {1ull, 8ull})
            for (uint32_t kt_slots : {2u, 3u, 16u}) {
                const L::KtNeed a = L::kt_need(total, n_texts, kt_slots, BSLOTS);
                CHECK(a.slots >= 64 && a.slots >= 2 * total && (a.slots & (a.slots - 1)) == 0);
                CHECK(a.slots == 64 || a.slots < 4 * total);
                // the check covers what a wide table then takes, whatever the distinct k-mers turn out to be
                for (uint64_t distinct : {total, total - total / 3, total / 2, (uint64_t)(total != 0)}) {
                    const uint64_t wide = L::kt_wide_buckets(distinct, kt_slots, BSLOTS) * 16 * BSLOTS;
                    CHECK(L::kt_wide_buckets(distinct, kt_slots, BSLOTS) * BSLOTS >= distinct * kt_slots);
                    CHECK(a.need >= a.slots * 8 + (n_texts + 1) * 8 + 16 + wide);
                }
                const uint64_t f1 = smallest_free_for(a.need);
                for (uint64_t f = f1 - 12; f <= f1 + 12; ++f)
                    CHECK(L::kt_build_fits(a, f, SPAN) == (a.slots <= SPAN && f >= f1));
                // 32-bit bucket hashing: 2^32 slots are the last
                CHECK(L::kt_build_fits(a, ~0ull, SPAN) == (a.slots <= SPAN));
                // the compact form, against the same answer
                for (uint32_t k : {12u, 21u, 23u})
                    for (uint32_t load8 : {10u, 35u, 90u})
                        for (uint64_t distinct : {total, total / 2}) {
                            if (distinct == 0) continue;
                            const L::KtCompact c = L::kt_compact(distinct, k, load8, SPAN);
                            CHECK(c.multi_cap == std::min<uint64_t>(distinct, (1ull << (63 - 2 * k)) - 2));
                            CHECK(c.nb8 * 8 * load8 >= distinct * 100 && (c.nb8 - 1) * 8 * load8 <= distinct * 100);
                            CHECK(c.addressable == (c.nb8 < SPAN));
                            // table, scratch array, counter, and the exact copy made while the scratch is alive
                            const uint64_t alive = a.keys_bytes + c.nb8 * 64 + c.multi_cap * 8 + 16 + c.multi_cap * 8;
                            CHECK(a.keys_bytes + c.bytes >= alive);
                            const uint64_t f2 = smallest_free_for(a.keys_bytes + c.bytes);
                            for (uint64_t f = f2 - 12; f <= f2 + 12; ++f) CHECK(L::kt_compact_fits(a, c, f) == (f >= f2));
                            // the second check fires on its own: the first passes, the compact form does not fit
                            if (f2 > f1 && load8 == 35 && kt_slots == 2 && a.slots <= SPAN) {
                                CHECK(L::kt_build_fits(a, f1, SPAN) && !L::kt_compact_fits(a, c, f1));
                                ++*compact_fired_default;
                            }
                        }
            }
    // nb8 against the bucket hash: 2^32 - 1 buckets are the last
    {
        uint64_t lo = 0, hi = 1ull << 40;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (L::kt_compact(mid, 12, 10, SPAN).nb8 >= SPAN) hi = mid;
            else lo = mid + 1;
        }
        CHECK(!L::kt_compact(lo, 12, 10, SPAN).addressable && L::kt_compact(lo - 1, 12, 10, SPAN).addressable);
        CHECK(L::kt_compact(lo - 1, 12, 10, SPAN).nb8 >= SPAN - 2);  // (1.25 buckets per k-mer: steps of 1 or 2)
    }
}

int main() {
    uint64_t n_layouts = 0, compact_fired_default = 0;
    free_memory_edges();
    offset_edges();
    sweep(&n_layouts);
    plane_edges();
    ktab_edges(&compact_fired_default);
    // the compact table's own check is reachable at the default tuning: say how often it was here
    CHECK(compact_fired_default > 0);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok layouts=%llu compact_check_alone=%llu\n", (unsigned long long)n_layouts,
                (unsigned long long)compact_fired_default);
    return 0;
}
