// Which kernel a scan launches, and with what launch shape: the one statement of the dispatch rule, as a pure
// function of plain facts. Host-only (no HIP include: tests/test_scan_plan_cpu.py compiles it with plain g++); the
// layout functions are constexpr, so device code calls them too.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

namespace speq_dev {
constexpr uint32_t WAVES_PER_BLOCK = 4;
constexpr uint32_t BLOCK_THREADS = 64 * WAVES_PER_BLOCK;
constexpr uint32_t LDS_HIST_MAX_G = 2048;
constexpr uint32_t QLUT_LEN = 42;  // phred42 ranks 0..41
// local mode, per block in LDS: {1 - 10^(-q/10), its reciprocal} for q = 0..41, then (k_scan_kt) the weight of a window
// of k bases that all have quality q
constexpr uint32_t QTAB_BYTES = QLUT_LEN * 24u;
enum { KM_GLOBAL = 0, KM_LOCAL = 1, KM_REF = 2 };

// Per-wave LDS: bases [buf_bytes] | qualities [buf_bytes] (local mode) | bad-mask words | N-mask words |
// base bit-plane words (bit 0 of every base's 2-bit code, then bit 1; k-mer table scans).
constexpr uint32_t staging_bytes(uint32_t k, uint32_t nwin) { return ((2u * (64u * nwin + k)) + 63u) & ~63u; }
constexpr uint32_t mask_words(uint32_t buf) { return buf / 64u + 1u; }
constexpr uint32_t wave_lds_bytes(uint32_t buf, bool local) { return buf * (local ? 2u : 1u) + 32u * mask_words(buf); }

// The histogram region at the start of a block's dynamic LDS (lds_hist: G <= LDS_HIST_MAX_G, else none): one u64 per
// group, two per group outside global mode, and with `totals` (k_scan, k_scan_kt) two more for {T, ambiguous};
// k_scan_ax keeps those two per wave instead. plan_scan requests this region and k_scan_ax carves it up through these
// two functions. k_scan and k_scan_kt (scan_kernels.hip) keep the same arithmetic typed out, totals = true: through
// the functions hipcc allocates the registers of their LDS-tally instantiations differently, and their device code
// is to stay as it is.
constexpr uint32_t hist_region_words(int mode, uint32_t G, bool lds_hist, bool totals) {
    return lds_hist ? (mode == KM_GLOBAL ? G : 2u * G) + (totals ? 2u : 0u) : 0u;
}
constexpr uint32_t hist_region_bytes(int mode, uint32_t G, bool lds_hist, bool totals) {
    return (hist_region_words(mode, G, lds_hist, totals) * 8u + 15u) & ~15u;
}
}  // namespace speq_dev

namespace speq {
using speq_dev::KM_GLOBAL;
using speq_dev::KM_LOCAL;
using speq_dev::KM_REF;
enum { VARIANT_K_SCAN = 0, VARIANT_K_SCAN_KT = 1, VARIANT_K_SCAN_AX = 2 };

// One instantiation of k_scan<MODE, PAIRED, LDS_HIST, NWIN, EM, KT>, k_scan_kt<MODE, PAIRED, LDS_HIST, EM, NW, CK> or
// k_scan_ax<MODE, PAIRED, LDS_HIST, EM, HW, STATS, SP>.
struct ScanVariant {
    int family = VARIANT_K_SCAN;
    int mode = KM_GLOBAL;   // KM_GLOBAL, KM_LOCAL, KM_REF (the reference-uniqueness pass)
    bool paired = false;
    bool lds_hist = false;  // G <= LDS_HIST_MAX_G: the tally in LDS; else global atomics
    bool em = false;        // the EM-histogram instantiation
    int width = 1;          // NWIN (1, 2, 4), NW (1, 2) or HW (1..4)
    bool kt = false;        // k_scan reads a k-mer table
    bool compact = false;   // k_scan_kt reads the compact 8-B-slot table (CK)
    bool sproof = false;    // k_scan_ax with the substitution-bitmap path (SP)
    bool stats = false;     // k_scan_ax's instrumented twin (STATS)
    // The value of tuning key "last_variant" (include/speq_scan.h): bits 0-1 family, 2-3 mode, 4 paired, 5 lds_hist,
    // 6 em, 7-9 width, 10 kt, 11 compact, 12 sproof, 13 stats.
    constexpr int pack() const {
        return family | mode << 2 | (int)paired << 4 | (int)lds_hist << 5 | (int)em << 6 | width << 7 | (int)kt << 10 |
               (int)compact << 11 | (int)sproof << 12 | (int)stats << 13;
    }
    static constexpr ScanVariant unpack(int x) {
        return {x & 3, x >> 2 & 3, (x >> 4 & 1) != 0, (x >> 5 & 1) != 0, (x >> 6 & 1) != 0, x >> 7 & 7,
                (x >> 10 & 1) != 0, (x >> 11 & 1) != 0, (x >> 12 & 1) != 0, (x >> 13 & 1) != 0};
    }
};

// The compile-time knob SPEQ_AX_SPROOF (ax_common.hpp; on unless a build sets it to 0 on the command line, as `make
// axknobs` does for `kv4`): without it the SP instantiations of k_scan_ax do not exist.
#if defined(SPEQ_AX_SPROOF) && !SPEQ_AX_SPROOF
constexpr bool AX_SPROOF_BUILT = false;
#else
constexpr bool AX_SPROOF_BUILT = true;
#endif

// The set of instantiations that exist: what is compiled, what may be launched, what is granted 160 KiB of LDS.
constexpr bool compiled(const ScanVariant& v) {
    const bool read_scan = v.mode == KM_GLOBAL || v.mode == KM_LOCAL;
    switch (v.family) {
    case VARIANT_K_SCAN:  // the pass: single, no EM, NWIN 1 or 2; reads: EM at NWIN 1, else 1, 2, and 4 for KT global
        if (v.compact || v.sproof || v.stats || v.mode > KM_REF) return false;
        if (v.mode == KM_REF) return !v.paired && !v.em && (v.width == 1 || v.width == 2);
        return v.em ? v.width == 1 : v.width == 1 || v.width == 2 || (v.width == 4 && v.kt && v.mode == KM_GLOBAL);
    case VARIANT_K_SCAN_KT:
        return read_scan && !v.kt && !v.sproof && !v.stats && (v.width == 1 || (v.width == 2 && !v.em));
    case VARIANT_K_SCAN_AX:  // SP at HW 1 only (k <= 32); the twin with the LDS tally and without an EM histogram only
        return read_scan && !v.kt && !v.compact && v.width >= 1 && v.width <= 4 &&
               (!v.sproof || (AX_SPROOF_BUILT && v.width == 1)) && (!v.stats || (v.lds_hist && !v.em));
    default:
        return false;
    }
}

// ... enumerated per family over every value of the fields (a 129th member would not compile)
struct VariantSet {
    int n = 0, packed[128] = {};
};
template <int FAMILY>
constexpr VariantSet compiled_set() {
    VariantSet s;
    for (int x = FAMILY; x < 1 << 14; x += 4)
        if (compiled(ScanVariant::unpack(x))) s.packed[s.n++] = x;
    return s;
}
template <int FAMILY>
inline constexpr VariantSet COMPILED = compiled_set<FAMILY>();
static_assert(COMPILED<VARIANT_K_SCAN>.n == 60 && COMPILED<VARIANT_K_SCAN_KT>.n == 48 &&
              COMPILED<VARIANT_K_SCAN_AX>.n == (AX_SPROOF_BUILT ? 100 : 80), "the scan kernels' instantiations");

// Runtime variant to template arguments. with_variant calls f(std::integral_constant<int, P>{}), P == v.pack(), for
// the member of FAMILY's compiled set that v is; f takes its template arguments from `constexpr ScanVariant V =
// ScanVariant::unpack(P)`. Only members of the set are ever instantiated (a guard by compiled() that cannot be left
// out), and a variant outside it throws: it never falls through to another kernel. for_each_compiled: f for every
// member.
template <int FAMILY, class F, size_t... I>
bool visit_compiled(int packed, bool all, F&& f, std::index_sequence<I...>) {
    constexpr const VariantSet& S = COMPILED<FAMILY>;
    return ((all || packed == S.packed[I] ? (f(std::integral_constant<int, S.packed[I]>{}), !all) : false) || ...);
}
template <int FAMILY, class F>
void for_each_compiled(F&& f) {
    (void)visit_compiled<FAMILY>(0, true, f, std::make_index_sequence<COMPILED<FAMILY>.n>{});
}
template <int FAMILY, class F>
void with_variant(const ScanVariant& v, F&& f) {
    constexpr std::make_index_sequence<COMPILED<FAMILY>.n> members{};
    if (v.family != FAMILY || !visit_compiled<FAMILY>(v.pack(), false, f, members))
        throw std::logic_error("scan dispatch: no compiled kernel for variant " + std::to_string(v.pack()));
}

// ---- the decision ----
enum { TABLE_NONE = 0, TABLE_WIDE = 1, TABLE_COMPACT = 2 };
constexpr uint64_t AX_MAX_UNITS = 1ull << 32;  // k_scan_ax indexes reads with 32 bits: the other kernels take more

struct ScanFacts {
    int mode = KM_GLOBAL;  // KM_REF: the reference-uniqueness pass
    bool paired = false, em = false, stats = false;
    uint32_t k = 0, G = 0;
    uint64_t units = 0;    // reads (not pairs); the pass: windows of the shard
    // tuning
    uint32_t ilp = 1, ilp_local = 1, ilp_kt = 0;
    bool kt_pipeline = true;
    uint32_t blocks_per_cu = 0, blocks_per_cu_kt = 0, blocks_per_cu_ax = 0;
    uint32_t grid_blocks = 0, grid_blocks_kt = 0, grid_blocks_ax = 0, ax_generations = 1, n_cus = 0;
    // what exists for this k
    bool ax_usable = false;      // the anchor structures (and, for an EM scan, their EM arrays)
    bool sproof_active = false;  // ... with a filled substitution bitmap that tuning "ax_sproof" turns on for k
    int table = TABLE_NONE;      // the k-mer table (not looked for when the anchor kernel takes the scan)
    uint32_t ax_wpb = 4, ax_wave_bytes = 0;  // k_scan_ax's waves per block, LDS per wave in this mode (ax_common.hpp)
};

struct ScanPlan {
    ScanVariant variant;
    int last_kernel = 0;      // tuning "last_kernel": 3 k_scan_ax, 2 k_scan_kt, 1 k_scan with KT, 0 k_scan, LF steps
    bool table_read = false;  // the kernel reads the k-mer table (it may exist and not be read: see below)
    uint32_t grid = 1;
    uint32_t grid_slots = 0;  // k_scan_ax: the grid is at most this many times its resident blocks per CU
    uint32_t buf_bytes = 0;   // UnitSrc::buf_bytes, the per-wave staging buffer
    size_t lds_bytes = 0;     // the dynamic LDS the kernel carves up
    size_t lds_launch = 0;    // ... and what the launch requests: padded so that only blocks_per_cu* blocks fit a CU
};

constexpr size_t lds_padded(size_t lds, uint32_t blocks_per_cu) {
    const size_t pad = blocks_per_cu > 0 ? (160u * 1024u) / blocks_per_cu : 0;
    return pad > lds ? pad & ~(size_t)15 : lds;
}

// No allocation, no lock, no HIP call: this runs on every launch.
inline ScanPlan plan_scan(const ScanFacts& f) {
    using namespace speq_dev;
    const bool ref = f.mode == KM_REF, local = f.mode == KM_LOCAL;
    ScanPlan p;
    ScanVariant& v = p.variant;
    v.mode = f.mode, v.paired = f.paired, v.lds_hist = f.G <= LDS_HIST_MAX_G, v.em = f.em && !ref;
    // The staging buffer is sized by the widest kernel any tuning of this replica could pick, not by the width
    // chosen below; the pass leaves "ilp_local" out.
    const uint32_t ilp_kt_or_2 = f.ilp_kt ? f.ilp_kt : 2u;
    p.buf_bytes = staging_bytes(f.k, std::max(std::max(f.ilp, ilp_kt_or_2), ref ? 0u : f.ilp_local));
    if (!ref && f.ax_usable && f.units < AX_MAX_UNITS) {
        v.family = VARIANT_K_SCAN_AX;
        // HW by k: 1 (k <= 32), 2 (k <= 64), 3 (k <= 96: the reference's default k = 70), 4 (k <= 128)
        v.width = f.k <= 32 ? 1 : f.k <= 64 ? 2 : f.k <= 96 ? 3 : 4;
        v.sproof = f.k <= 32 && f.sproof_active;
        // the instrumented twin exists with the LDS tally and without an EM histogram only (the entry point refuses
        // the rest before it gets here); otherwise the plain kernel runs and adds no counters
        v.stats = f.stats && v.lds_hist && !v.em;
        p.last_kernel = 3;
        p.lds_bytes = hist_region_bytes(f.mode, f.G, v.lds_hist, false) + (local ? QTAB_BYTES : 0u) +
                      (size_t)f.ax_wpb * f.ax_wave_bytes;
        p.lds_launch = lds_padded(p.lds_bytes, f.blocks_per_cu_ax);
        const uint64_t blocks = (f.units + 64u * f.ax_wpb - 1) / (64u * f.ax_wpb);
        p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, f.grid_blocks_ax));
        p.grid_slots = f.n_cus * f.ax_generations;
        return p;
    }
    // A table that exists for k sets the launch shape ("grid_blocks_kt", "blocks_per_cu_kt"); whether it is read
    // chooses the kernel. A compact table is read by the pipelined kernel only, so not by the pass, and not with
    // "kt_pipeline" 0 or "ilp_kt" 4: those scans of this k take LF steps under the table's launch shape.
    const bool table_exists = f.table != TABLE_NONE;
    const bool pipelined = !ref && f.ilp_kt <= 2 && f.kt_pipeline;
    p.table_read = f.table == TABLE_WIDE || (f.table == TABLE_COMPACT && pipelined);
    if (p.table_read && pipelined) {
        v.family = VARIANT_K_SCAN_KT;
        v.compact = f.table == TABLE_COMPACT;
        v.width = v.em ? 1 : (int)(f.ilp_kt ? f.ilp_kt : (v.compact ? 1u : 2u));
    } else {
        v.family = VARIANT_K_SCAN;
        v.kt = p.table_read;
        const uint32_t ilp = v.kt ? ilp_kt_or_2 : (local ? f.ilp_local : f.ilp);
        v.width = v.em ? 1 : (v.kt && f.mode == KM_GLOBAL && ilp == 4) ? 4 : ilp >= 2 ? 2 : 1;
    }
    p.last_kernel = v.family == VARIANT_K_SCAN_KT ? 2 : v.kt ? 1 : 0;
    p.lds_bytes = hist_region_bytes(f.mode, f.G, v.lds_hist, true) + (local ? QTAB_BYTES : 0u) +
                  (size_t)WAVES_PER_BLOCK * wave_lds_bytes(p.buf_bytes, local);
    p.lds_launch = lds_padded(p.lds_bytes, table_exists ? f.blocks_per_cu_kt : f.blocks_per_cu);
    // >= 4 units (pairs of a paired scan; the pass: 256 windows) per wave; the grid capped (default 2x the 8
    // resident blocks x 256 CUs)
    const uint64_t work = ref ? (f.units + 255) / 256 : f.paired ? f.units / 2 : f.units;
    const uint64_t blocks = (work + 4 * WAVES_PER_BLOCK - 1) / (4 * WAVES_PER_BLOCK);
    const uint32_t cap = table_exists ? f.grid_blocks_kt : f.grid_blocks;
    p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, cap));
    return p;
}
}  // namespace speq
