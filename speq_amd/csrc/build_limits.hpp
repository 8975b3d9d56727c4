// Every decision the library takes because device memory is short or an index is large ("Size and
// memory decisions"), as plain functions of integers. Host-only, no HIP include: build_ax, ensure_ax_em (ax_scan.hip),
// build_ktab and speq_device_open (scan_kernels.hip) call these, and tests/build_limits_check.cpp checks each
// inequality on both sides of its edge without a GPU.
//
// `free_b` is what speq_dev::mem::free_bytes() answered; `limit` is speq_dev::mem::offset_limit(): 2^32, the span of a
// 32-bit buffer offset, unless a test lowered it (speq_debug_offset_limit).
#pragma once
#include <algorithm>
#include <cstdint>

namespace speq::limits {

constexpr uint64_t OFFSET_SPAN = 1ull << 32;
// the offset a lane with nothing to load is given (scan_device.hpp: OOB): it must lie outside every descriptor
constexpr uint64_t OOB_SLACK = 16;
constexpr uint64_t AX_SLACK = 64;  // build_ax keeps its tables this far below the span

// a tenth of the free memory stays free (other processes, the runtime's own allocations)
inline uint64_t usable(uint64_t free_b) { return free_b / 10 * 9; }
inline bool fits(uint64_t need, uint64_t free_b) { return need <= usable(free_b); }

// ---- build_ax ----
struct AxNeed {
    uint64_t nw64;        // 64-bit words of the 2-bit text's bitmap (+ 4 of slack)
    uint64_t n_gran;      // granules of 32 text positions
    uint64_t gran_bytes;
    uint64_t need;        // gran, codes, owner, text2 + tbad, table + filter (bounds)
};
inline AxNeed ax_need(uint64_t n) {
    AxNeed r;
    r.nw64 = (n + 63) / 64 + 4;
    r.n_gran = (n + 255) / 32 + 2;
    r.gran_bytes = r.n_gran * 16;
    r.need = r.gran_bytes + n + (n + 64) * 4 + r.nw64 * 24 + n * 12;
    return r;
}
// first check: false defers the whole build (transient)
inline bool ax_build_fits(const AxNeed& a, uint64_t free_b) { return fits(a.need, free_b); }
// second check: the suffix sort's buffer and temporaries (60 B per symbol) beside everything else; false: the first
// claimant of an interval represents it
inline bool ax_sort_fits(uint64_t n, const AxNeed& a, uint64_t free_b) { return n * 60 + a.need < usable(free_b); }

// m of the m-mer filter: the smallest m >= 12 with 4^m >= 200 n, and only when one probe covers at least `cover`
// windows (k - m + 1); 0: none
inline uint32_t ax_mfilter_m(uint64_t n, uint32_t k, uint32_t cover) {
    uint32_t m = 12;
    while (m < 32u && (double)(1ull << (2u * m)) < 200.0 * (double)n) ++m;
    return k + 1u >= m + cover ? m : 0u;
}

// The anchor table's allocation: nb buckets of 64 B, then the m-mer filter (nmf words + 16 B), then the substitution
// bitmap (s_words words + 16 B). Each part must be addressable by a 32-bit buffer offset.
struct AxLayout {
    bool refused = false;  // the buckets or the k-mer filter outgrow the span: structural, never retried
    uint64_t nb = 0, nf = 0, nmf = 0, s_off = 0, s_words = 0, s_bytes = 0, atab_bytes = 0;
    uint32_t m = 0;
};
inline bool ax_beyond(uint64_t bytes, uint64_t limit) { return bytes >= limit - AX_SLACK; }
// filter_bits: Bloom bits per k-mer; m: ax_mfilter_m; sproof: the bitmap is compiled in
inline AxLayout ax_layout(uint64_t n, uint32_t k, uint64_t distinct, uint64_t n_texts, uint32_t load,
                          uint32_t filter_bits, uint32_t m, bool sproof, uint64_t limit) {
    AxLayout a;
    a.nf = std::max<uint64_t>(1, distinct * filter_bits / 64);
    a.nb = std::max<uint64_t>(1, (uint64_t)((double)distinct * 100.0 / (8.0 * load)) + 1);
    a.m = m;
    a.nmf = m ? std::max<uint64_t>(1, (distinct + n_texts * k) * filter_bits / 64) : 0;
    // the m-mer filter goes first: a table without it still answers every window
    if (a.m && ax_beyond(a.nb * 64u + a.nmf * 8u + 16u, limit)) a.m = 0, a.nmf = 0;
    if (ax_beyond(a.nb * 64u, limit) || ax_beyond(a.nf * 8u, limit)) {
        AxLayout r;
        r.refused = true;
        return r;
    }
    a.s_off = a.nb * 64u + (a.m ? a.nmf * 8u + 16u : 0u);
    a.s_words = sproof ? ((n + 255) / 256) * 4 : 0;
    if (ax_beyond(a.s_off + a.s_words * 8u + 16u, limit)) a.s_words = 0;
    a.s_bytes = a.s_words ? a.s_words * 8u + 16u : 0u;
    a.atab_bytes = a.s_off + a.s_bytes;
    return a;
}
// third check: false defers the table and the filter (transient)
inline bool ax_table_fits(const AxLayout& a, uint64_t free_b) { return fits(a.atab_bytes + a.nf * 8, free_b); }
// the length of the descriptor k_scan_ax builds over the table's allocation (rs_atab): with the bitmap for the
// instantiations that read it, else up to the m-mer filter's end (mfilter: tuning "ax_mproof" is not 0)
inline uint32_t ax_atab_desc_len(const AxLayout& a, bool sproof_variant, bool mfilter) {
    if (sproof_variant && a.s_bytes != 0u) return (uint32_t)a.s_off + (uint32_t)a.s_bytes;
    return (uint32_t)(a.nb * 64u + (mfilter && a.m != 0u ? a.nmf * 8u + 16u : 0u));
}

// ensure_ax_em: mlo and mhi, 4 B per text position each; false sends EM scans to the other kernels
inline uint64_t ax_em_bytes(uint64_t n) { return (n + 64) * 8; }
inline bool ax_em_fits(uint64_t n, uint64_t free_b) { return fits(ax_em_bytes(n), free_b); }

// ---- build_ktab ----
inline uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
struct KtNeed {
    uint64_t slots;       // the key set: a power of two >= 2 x the windows
    uint64_t keys_bytes;  // the key set, the windows' prefix sums per text, the counter: alive until the fill ends
    uint64_t need;        // those + a wide table of kt_slots slots per window (every window a distinct k-mer)
};
// the buckets (bslots slots of 16 B) of a wide table of `distinct` k-mers
inline uint64_t kt_wide_buckets(uint64_t distinct, uint32_t kt_slots, uint32_t bslots) {
    return next_pow2(std::max<uint64_t>(1, (distinct * kt_slots + bslots - 1) / bslots));
}
inline KtNeed kt_need(uint64_t total, uint64_t n_texts, uint32_t kt_slots, uint32_t bslots) {
    KtNeed r;
    r.slots = next_pow2(std::max<uint64_t>(2 * total, 64));
    r.keys_bytes = r.slots * 8 + (n_texts + 1) * 8 + 16;
    r.need = r.keys_bytes + kt_wide_buckets(total, kt_slots, bslots) * 16 * bslots;
    return r;
}
// first check: false leaves the k to LF steps (no table; cached for the replica's life)
inline bool kt_build_fits(const KtNeed& a, uint64_t free_b, uint64_t limit) {
    return a.slots <= limit && fits(a.need, free_b);
}
struct KtCompact {
    uint64_t nb8;        // buckets of 64 B for the load factor kt_load8
    uint64_t multi_cap;  // the scratch array of multi-group k-mers: every distinct k-mer, up to the payload bits
    uint64_t bytes;      // both, the counter and the exact copy of the scratch array (worst case: all of it)
    bool addressable;    // nb8 fits the 32-bit bucket hash
};
inline KtCompact kt_compact(uint64_t distinct, uint32_t k, uint32_t kt_load8, uint64_t limit) {
    KtCompact c;
    const uint32_t pbits = 64u - 2u * k;  // k <= 23: at least 18
    c.multi_cap = std::min<uint64_t>(distinct, (1ull << (pbits - 1u)) - 2u);
    c.nb8 = std::max<uint64_t>(1, (uint64_t)((double)distinct * 100.0 / (8.0 * kt_load8)) + 1);
    c.bytes = c.nb8 * 64 + 2 * std::max<uint64_t>(c.multi_cap, 1) * 8 + 16;
    c.addressable = c.nb8 < limit;
    return c;
}
// second check, for a compact table only and against the same answer as the first (the key set is still alive):
// false leaves the k to LF steps. A compact table takes (800 / kt_load8 + 16) B per distinct k-mer, a wide one at
// least 16 kt_slots B per window: the check can fire where nearly every window is a distinct k-mer and kt_load8 is
// below 800 / (16 kt_slots - 16) (50 at kt_slots = 2, so at the default 35 too).
inline bool kt_compact_fits(const KtNeed& a, const KtCompact& c, uint64_t free_b) {
    return fits(a.keys_bytes + c.bytes, free_b);
}

// ---- speq_device_open ----
// Which plane families a replica of nb blocks (96 positions each) can address. lf_step forms plane_id * nb * 16 +
// blk * 16 in 32 bits and make_rsrc the family's size; both stay exact, and the OOB offset stays out of range, iff
// planes * nb * 16 <= span - 16. Three-symbol planes (64) wrap from nb = 2^22, two-symbol planes (16) from 2^24;
// the one-symbol planes (5) and the run bitvector (1) cannot below 2^31 symbols. The search uses the two-symbol
// planes for what the three-symbol steps leave over, so occ3 needs occ2.
struct PlaneFamilies {
    bool occ, occ2, occ3;
};
inline bool planes_addressable(uint64_t planes, uint64_t nb, uint64_t limit) {
    return planes * nb * 16 <= limit - OOB_SLACK;
}
inline PlaneFamilies plane_families(uint64_t nb, bool has_occ2, bool has_occ3, uint64_t limit) {
    PlaneFamilies p;
    p.occ = planes_addressable(5, nb, limit);
    p.occ2 = has_occ2 && p.occ && planes_addressable(16, nb, limit);
    p.occ3 = has_occ3 && p.occ2 && planes_addressable(64, nb, limit);
    return p;
}

}  // namespace speq::limits
