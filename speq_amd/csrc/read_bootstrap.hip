// Read bootstrap (speq_bootstrap_*): the scan's counter vector under B Poisson(1) resamplings of the
// reads, in one pass. Every unit (a read, or the pair 2u, 2u + 1) gets B integer weights that are a pure function of
// (seed, unit index, replicate), and its passing windows, its ambiguity flag and its per-group unique windows are added,
// times each weight, to B + 1 counter vectors (replicate 0 is the sample itself: every weight is 1). A diagnostic pass
// beside the scan kernels, shaped like the per-unit report (read_report.hip): every passing window gets an exact
// backward search (search_lds), no per-k structure is used, and nothing here is on the hot path of `speq scan`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "em.hpp"
#include "window_pass.hpp"

struct speq_bootstrap {
    speq_device_index* dev = nullptr;
    speq_scan_params params{};  // k, phred_cutoff, paired and mode, fixed at create
    uint32_t B = 0;             // replicates; the accumulators hold R = B + 1 rows
    uint32_t G = 0;
    uint64_t seed = 0;
    // accumulators with the replicates contiguous: counts cell (c, b) at c * R + b for c < G + 2, weights cell (g, b)
    // at g * R + b (the 64 lanes of a wave add to consecutive addresses); finalize transposes them on the host
    speq_dev::DevPtr<unsigned long long> d_counts;
    speq_dev::DevPtr<double> d_weights;  // local mode only
    std::atomic<uint32_t> lds_path{0};
    std::atomic<uint64_t> units_added{0};
    // an attached EM histogram (speq_bootstrap_attach_em): the sorted interval starts with the slot of
    // each one's merged row, and M, u64 [n_rows][R], cell (slot, b) at slot * R + b
    bool em_attached = false;
    uint64_t em_rows = 0;
    uint32_t em_m = 0, em_lds_rows = 0;
    speq_dev::DevPtr<uint32_t> d_em_lo, d_em_slot;
    speq_dev::DevPtr<unsigned long long> d_em_mult, d_em_missed;
    std::vector<uint32_t> em_slot_of_row;
};

namespace {

using namespace speq_dev;

// ---- the weight function (integer only; tests/bootstrap_model.py restates it) ----
constexpr uint64_t GAMMA = 0x9e3779b97f4a7c15ull;
constexpr uint32_t N_THRESHOLDS = 21;
// splitmix64's finaliser
__host__ __device__ inline uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t unit_key(uint64_t seed, uint64_t unit) { return mix(seed + GAMMA * (unit + 1ull)); }
__host__ __device__ inline uint64_t draw(uint64_t key, uint32_t b) { return mix(key + GAMMA * (uint64_t)b); }

// C_j = floor(2^64 * e^-1 * sum_{i <= j} 1 / i!), j = 0 .. 20 (computed with 80-digit decimals): a uniform 64-bit h
// has weight w(h) = #{j : h >= C_j}, so P(w = j) is Poisson(1)'s to within 2^-64. C_20 = 2^64 - 1 is the last
// threshold a 64-bit h can reach: the largest weight is 21. The thresholds ascend, so the count stops at the first one
// above h: five draws in six end below C_1 (two compares), one in 270 goes past C_4.
__host__ __device__ inline uint32_t weight_of(uint64_t h) {
    constexpr uint64_t C[N_THRESHOLDS] = {
        0x5e2d58d8b3bcdf1aull, 0xbc5ab1b16779be35ull, 0xeb715e1dc1582dc2ull, 0xfb23979734a252f1ull,
        0xff1025f59174dc3dull, 0xffd90f3ba4055e19ull, 0xfffa8b71fc72c913ull, 0xffff540c0914b3c9ull,
        0xffffed1f4aa8f120ull, 0xfffffe216e641462ull, 0xffffffd4d85d3183ull, 0xfffffffc6da262b4ull,
        0xffffffffba12d178ull, 0xfffffffffb07c64cull, 0xffffffffffab8ea5ull, 0xfffffffffffabe22ull,
        0xffffffffffffb11aull, 0xfffffffffffffba1ull, 0xffffffffffffffc5ull, 0xfffffffffffffffdull,
        0xffffffffffffffffull};
    uint32_t w = 0;
    while (w < N_THRESHOLDS && h >= C[w]) ++w;
    return w;
}
// replicate b's weight of the unit with key `key` (b = 0: the sample itself)
__device__ __forceinline__ uint32_t rep_weight(uint64_t key, uint32_t b) { return b == 0u ? 1u : weight_of(draw(key, b)); }

// ---- accumulation ----
// A block's accumulators go to LDS when they fit LDS_BUDGET together with the tile search's regions: 64 KiB, the most a
// launch takes without opting in to more, which leaves two blocks resident in a CU's 160 KiB. Nobody has measured the
// two paths against each other; the LDS one is chosen where it fits because B * (G + 2) cells shared by every wave of
// the grid serialise global atomics on a few hundred addresses, while a block's LDS takes them at LDS rate and the
// block then adds each non-zero cell to HBM once.
constexpr uint32_t LDS_BUDGET = 64u << 10;
inline uint64_t acc_bytes(uint32_t R, uint32_t G, bool local) { return 8ull * R * ((uint64_t)G + 2u + (local ? G : 0u)); }
inline bool fits_lds(uint32_t R, uint32_t G, bool local, uint32_t k) {
    return acc_bytes(R, G, local) + (uint64_t)WAVES_PER_BLOCK * wave_bytes(k) <= LDS_BUDGET;
}

// What a launch with an attached histogram takes beside the counters: lo[m] ascending, slot[m], the first `lds_rows`
// slots' cells in the block's LDS and every other slot's in mult
struct EmDev {
    const uint32_t* lo;
    const uint32_t* slot;
    unsigned long long* mult;
    unsigned long long* missed;
    uint32_t m, lds_rows;
};
// rows of an attached histogram whose R cells a block keeps in LDS: what is left of LDS_BUDGET after the tile search's
// regions and, when they take the LDS path, the counters
inline uint32_t em_lds_rows(uint64_t n_rows, uint32_t R, uint32_t G, bool local, uint32_t k) {
    const uint64_t taken = (uint64_t)WAVES_PER_BLOCK * wave_bytes(k) + (fits_lds(R, G, local, k) ? acc_bytes(R, G, local) : 0u);
    return (uint32_t)std::min<uint64_t>(n_rows, taken >= LDS_BUDGET ? 0u : (LDS_BUDGET - taken) / (8ull * R));
}

// sum over the wave of v (every lane gets it)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One wave64 owns one unit and walks each mate in tiles of 64 window starts; lane j searches window tile + j
// (search_tile, window_pass.hpp). Lanes then stride over the replicates (b = lane, lane + 64, ...): in the wave-uniform
// round of each distinct group g of the tile every lane adds w_b * (windows of the tile unique to g) to cell (2 + g, b),
// and after the unit's tiles w_b * passing to cell (0, b) and, for a unit with two or more groups, w_b to cell (1, b).
// The weights are recomputed where they are used (two 64-bit multiplies and a few compares). LOCAL: a lane also has
// its window's Phred weight x (the scan's chain of divisions), and the round adds w_b * (sum of x over the group's
// windows of the tile) to the weights cell (g, b). EM (an attached histogram): a lane whose window lies in two or more
// groups looks its interval start up in E.lo (binary search; the table is L2-resident) and takes the slot of its merged
// row, and one more wave-uniform loop, a round per distinct slot of the tile, adds w_b * (windows of the tile in the
// slot) to cell (slot, b): in the block's LDS for the slots below E.lds_rows, which are flushed with the counters, and
// in E.mult for the rest. A start that the table does not hold is counted in *E.missed, once per tile.
template <bool PAIRED, bool LOCAL, bool LDS_ACC, bool EM>
__global__ __launch_bounds__(BLOCK_THREADS) void k_read_bootstrap(
    const DevView I, const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, const uint64_t* __restrict__ off,
    uint64_t n_units, uint64_t first_unit, uint32_t k, uint32_t cutoff, uint32_t R, uint64_t seed,
    const double* __restrict__ qlut, unsigned long long* __restrict__ g_counts, double* __restrict__ g_weights,
    const EmDev E) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint16_t* cnt = wave_cnt(lds, wave, k);
    unsigned char* sym = wave_sym(lds, wave, k);
    const uint32_t G = I.G;
    const uint32_t n_cells = (G + 2u) * R, n_wcells = LOCAL ? G * R : 0u;
    unsigned long long* acc = g_counts;
    double* wacc = g_weights;
    if (LDS_ACC) {
        acc = reinterpret_cast<unsigned long long*>(lds + WAVES_PER_BLOCK * wave_bytes(k));
        wacc = reinterpret_cast<double*>(acc + n_cells);
        for (uint32_t i = threadIdx.x; i < n_cells; i += BLOCK_THREADS) acc[i] = 0ull;
        for (uint32_t i = threadIdx.x; i < n_wcells; i += BLOCK_THREADS) wacc[i] = 0.0;
        __syncthreads();
    }
    unsigned long long* hot = nullptr;
    if (EM) {
        hot = reinterpret_cast<unsigned long long*>(lds + WAVES_PER_BLOCK * wave_bytes(k)) +
              (LDS_ACC ? n_cells + n_wcells : 0u);
        for (uint32_t i = threadIdx.x; i < E.lds_rows * R; i += BLOCK_THREADS) hot[i] = 0ull;
        __syncthreads();
    }
    const Rsrc Rs = make_rsrc(I);
    for (uint64_t u = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; u < n_units;
         u += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t key = unit_key(seed, first_unit + u);
        uint32_t passing = 0, first = 0xFFFFFFFFu;
        bool amb = false;
        for (uint32_t m = 0; m < (PAIRED ? 2u : 1u); ++m) {
            const uint64_t r = PAIRED ? 2u * u + m : u;
            const uint64_t beg = off[r], len = off[r + 1] - beg;
            if (len < k) continue;
            const uint64_t nwin = len - k + 1u;
            for (uint64_t tile = 0; tile < nwin; tile += 64u) {
                const uint32_t span = (uint32_t)min((uint64_t)(64u + k - 1u), len - tile);  // staged positions
                uint32_t lo = 0;
                bool pass;
                int res = search_tile(I, Rs, sym, cnt, span, k, tile + lane < nwin, lane, lo,
                                      SPEQ_READ_TILE_AT(seq, qual, beg + tile, cutoff), &pass);
                constexpr uint32_t NO_SLOT = 0xFFFFFFFFu, MISSED = 0xFFFFFFFEu;
                uint32_t slot = NO_SLOT;
                if (EM && res == -2) {
                    uint32_t a = 0, e = E.m;
                    while (a < e) {
                        const uint32_t mid = (a + e) >> 1;
                        if (E.lo[mid] < lo) a = mid + 1u;
                        else e = mid;
                    }
                    slot = a < E.m && E.lo[a] == lo ? E.slot[a] : MISSED;
                }
                if ((uint32_t)res >= G) res = -1;  // (also every negative result)
                passing += (uint32_t)__popcll(__ballot(pass));
                double x = 0.0;
                if (LOCAL && res >= 0) {  // the window passed: every quality is above the cutoff, so never 0
                    const uint8_t* q = qual + beg + tile + lane;
                    x = 1.0;
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint32_t c = (uint32_t)min(max((int32_t)q[i] - 33, 0), 41);
                        x = div_rn(x, qlut[2u * c], qlut[2u * c + 1u]);  // == x / qlut[2 c]
                    }
                }
                uint64_t rest = __ballot(res >= 0);  // wave-uniform: one round per distinct group of the tile
                while (rest != 0ull) {
                    const int g = __shfl(res, __builtin_ctzll(rest));
                    const uint64_t of_g = __ballot(res == g);
                    rest &= ~of_g;
                    if (first == 0xFFFFFFFFu) first = (uint32_t)g;
                    else if (first != (uint32_t)g) amb = true;
                    const uint32_t n_g = (uint32_t)__popcll(of_g);
                    double x_g = 0.0;
                    if (LOCAL) x_g = wave_sum(res == g ? x : 0.0);
                    for (uint32_t b = lane; b < R; b += 64u) {
                        const uint32_t w = rep_weight(key, b);
                        if (w == 0u) continue;
                        atomicAdd(&acc[(2u + (uint32_t)g) * R + b], (unsigned long long)w * n_g);
                        if (LOCAL) atomicAdd(&wacc[(uint32_t)g * R + b], (double)w * x_g);
                    }
                }
                if (EM) {
                    const uint64_t miss = __ballot(slot == MISSED);
                    if (miss != 0ull && lane == 0u) atomicAdd(E.missed, (unsigned long long)__popcll(miss));
                    uint64_t left = __ballot(slot < MISSED);  // wave-uniform: one round per distinct slot of the tile
                    while (left != 0ull) {
                        const uint32_t s = (uint32_t)__shfl((int)slot, __builtin_ctzll(left));
                        const uint64_t of_s = __ballot(slot == s);
                        left &= ~of_s;
                        const uint32_t n_s = (uint32_t)__popcll(of_s);
                        unsigned long long* cell = s < E.lds_rows ? hot + s * R : E.mult + (uint64_t)s * R;
                        for (uint32_t b = lane; b < R; b += 64u) {
                            const uint32_t w = rep_weight(key, b);
                            if (w == 0u) continue;
                            atomicAdd(&cell[b], (unsigned long long)w * n_s);
                        }
                    }
                }
            }
        }
        if (passing != 0u)
            for (uint32_t b = lane; b < R; b += 64u) {
                const uint32_t w = rep_weight(key, b);
                if (w == 0u) continue;
                atomicAdd(&acc[b], (unsigned long long)w * passing);
                if (amb) atomicAdd(&acc[R + b], (unsigned long long)w);
            }
    }
    if (LDS_ACC) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_cells; i += BLOCK_THREADS)
            if (acc[i] != 0ull) atomicAdd(&g_counts[i], acc[i]);
        for (uint32_t i = threadIdx.x; i < n_wcells; i += BLOCK_THREADS)
            if (wacc[i] != 0.0) atomicAdd(&g_weights[i], wacc[i]);
    }
    if (EM) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < E.lds_rows * R; i += BLOCK_THREADS)
            if (hot[i] != 0ull) atomicAdd(&E.mult[i], hot[i]);
    }
}

using Kernel = void (*)(const DevView, const uint8_t*, const uint8_t*, const uint64_t*, uint64_t, uint64_t, uint32_t,
                        uint32_t, uint32_t, uint64_t, const double*, unsigned long long*, double*, const EmDev);
template <bool PAIRED, bool LOCAL>
Kernel pick(bool lds, bool em) {
    if (em) return lds ? k_read_bootstrap<PAIRED, LOCAL, true, true> : k_read_bootstrap<PAIRED, LOCAL, false, true>;
    return lds ? k_read_bootstrap<PAIRED, LOCAL, true, false> : k_read_bootstrap<PAIRED, LOCAL, false, false>;
}
Kernel pick(bool paired, bool local, bool lds, bool em) {
    if (paired) return local ? pick<true, true>(lds, em) : pick<true, false>(lds, em);
    return local ? pick<false, true>(lds, em) : pick<false, false>(lds, em);
}

void check_create_args(const char* who, const speq_scan_params* p, uint32_t replicates) {
    if (!p) throw std::invalid_argument(std::string(who) + ": null params");
    speq::check_report_k(who, p->k);
    if (replicates < 1 || replicates > SPEQ_BOOTSTRAP_MAX_REPLICATES)
        throw std::invalid_argument(std::string(who) + ": replicates must be in [1, " +
                                    std::to_string(SPEQ_BOOTSTRAP_MAX_REPLICATES) + "]");
}

bool is_local(const speq_scan_params& p) { return p.mode == SPEQ_MODE_LOCAL; }

void create_impl(speq_device_index* d, const speq_scan_params* p, uint32_t replicates, uint64_t seed,
                 speq_bootstrap** out) {
    const char* who = "speq_bootstrap_create";
    check_create_args(who, p, replicates);
    if (!d) throw std::invalid_argument(std::string(who) + ": null device index");
    if (!out) throw std::invalid_argument(std::string(who) + ": null output");
    DeviceGuard g(d->device);
    auto b = std::make_unique<speq_bootstrap>();
    b->dev = d;
    b->params = *p;
    b->B = replicates;
    b->G = d->G;
    b->seed = seed;
    const uint64_t R = (uint64_t)replicates + 1u;
    const size_t cb = (size_t)(R * (b->G + 2u) * 8u), wb = (size_t)(R * b->G * 8u);
    b->d_counts = DevPtr<unsigned long long>::alloc(cb / 8u, who);
    if (is_local(*p)) b->d_weights = DevPtr<double>::alloc(wb / 8u, who);
    SyncOnExit sync(d->stream);  // (declared after b: the stream is idle before a throw frees the handle's arrays)
    HIP_OK(hipMemsetAsync(b->d_counts.get(), 0, cb, d->stream));
    if (b->d_weights) HIP_OK(hipMemsetAsync(b->d_weights.get(), 0, std::max<size_t>(wb, 16), d->stream));
    // the adds come on the callers' streams: the zeros are in place before the handle exists
    HIP_OK(hipStreamSynchronize(d->stream));
    *out = b.release();
}

void add_device_impl(speq_bootstrap* b, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_offsets,
                     uint64_t n_reads, uint64_t first_unit, hipStream_t st) {
    const char* who = "speq_bootstrap_add_reads_device";
    if (n_reads > 0 && (!d_seq || !d_qual || !d_offsets)) throw std::invalid_argument(std::string(who) + ": null buffer");
    if (!b) throw std::invalid_argument(std::string(who) + ": null handle");
    const bool paired = b->params.paired != 0;
    if (paired && (n_reads & 1))
        throw std::invalid_argument(std::string(who) + ": a paired handle needs an even record count");
    const uint64_t n_units = paired ? n_reads / 2 : n_reads;
    if (n_units == 0) return;
    speq_device_index* d = b->dev;
    DeviceGuard g(d->device);
    const uint32_t k = b->params.k, R = b->B + 1u;
    const bool local = is_local(b->params), lds_acc = fits_lds(R, b->G, local, k);
    const DevView v = speq::search_view(d, k);
    const EmDev E{b->d_em_lo.get(), b->d_em_slot.get(), b->d_em_mult.get(), b->d_em_missed.get(),
                  b->em_m, b->em_lds_rows};
    const size_t lds = (size_t)WAVES_PER_BLOCK * wave_bytes(k) + (lds_acc ? (size_t)acc_bytes(R, b->G, local) : 0) +
                       (size_t)E.lds_rows * R * 8u;
    // LDS path (the counters', or an attached histogram's hot rows alone): a block zeroes and flushes its accumulators
    // once, so the grid is a few blocks per CU and the waves stride over the units; global path: as the report's
    const bool lds_grid = lds_acc || E.lds_rows != 0u;
    const uint64_t want = (n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const uint64_t per_cu = std::min<uint64_t>(std::max<uint64_t>((160u << 10) / lds, 2), 8);  // resident blocks
    const uint64_t blocks = std::min<uint64_t>(want, lds_grid ? per_cu * std::max(d->n_cus, 1u) : 16384u);
    hipLaunchKernelGGL(pick(paired, local, lds_acc, b->em_attached), dim3((uint32_t)blocks), dim3(BLOCK_THREADS), lds,
                       st, v, d_seq, d_qual, d_offsets, n_units, first_unit, k, b->params.phred_cutoff, R, b->seed,
                       d->d_qlut, b->d_counts.get(), b->d_weights.get(), E);
    HIP_OK(hipGetLastError());
    b->lds_path = lds_acc ? 1u : 0u;
    b->units_added += n_units;
}

void add_host_impl(speq_bootstrap* b, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                   uint64_t n_reads, uint64_t first_unit) {
    const char* who = "speq_bootstrap_add_reads";
    // (the handle last: every check of the arrays is made before anything of the device is touched)
    if (n_reads > 0 && !offsets) throw std::invalid_argument(std::string(who) + ": null offsets");
    speq::check_host_reads(who, seq, qual, offsets, n_reads);
    if (!b) throw std::invalid_argument(std::string(who) + ": null handle");
    const uint32_t per = b->params.paired ? 2u : 1u;
    if (n_reads % per) throw std::invalid_argument(std::string(who) + ": a paired handle needs an even record count");
    if (n_reads == 0) return;
    speq_device_index* d = b->dev;
    DeviceGuard g(d->device);
    // the batches hold whole units; a batch's first record r0 is unit first_unit + r0 / per
    for_staged_batches(who, d, seq, qual, offsets, n_reads, per,
                       [&](const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint64_t r0, uint64_t n) {
                           add_device_impl(b, d_seq, d_qual, d_off, n, first_unit + r0 / per, d->stream);
                       });
}

void finalize_impl(speq_bootstrap* b, uint64_t* counts, double* weights) {
    const char* who = "speq_bootstrap_finalize";
    if (!b) throw std::invalid_argument(std::string(who) + ": null handle");
    if (!counts) throw std::invalid_argument(std::string(who) + ": null output");
    const bool local = is_local(b->params);
    if (local && !weights) throw std::invalid_argument(std::string(who) + ": a local handle needs the weights output");
    speq_device_index* d = b->dev;
    DeviceGuard g(d->device);
    HIP_OK(hipDeviceSynchronize());  // the adds of every stream of the device have completed
    const uint32_t R = b->B + 1u, G = b->G, C = G + 2u;
    std::vector<uint64_t> hc((size_t)R * C);
    HIP_OK(hipMemcpy(hc.data(), b->d_counts.get(), hc.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < C; ++c)
        for (uint32_t r = 0; r < R; ++r) counts[(size_t)r * C + c] = hc[(size_t)c * R + r];
    if (local && G) {
        std::vector<double> hw((size_t)R * G);
        HIP_OK(hipMemcpy(hw.data(), b->d_weights.get(), hw.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t c = 0; c < G; ++c)
            for (uint32_t r = 0; r < R; ++r) weights[(size_t)r * G + c] = hw[(size_t)c * R + r];
    }
}

// ---- an attached EM histogram ----
void attach_em_impl(speq_bootstrap* b, const speq_em* em) {
    const char* who = "speq_bootstrap_attach_em";
    if (!b || !em) throw std::invalid_argument(std::string(who) + ": null argument");
    if (!em->finalized) throw std::invalid_argument(std::string(who) + ": histogram not finalized");
    if (em->dev != b->dev || em->G != b->G)
        throw std::invalid_argument(std::string(who) + ": the histogram is of another replica");
    if (b->em_attached) throw std::invalid_argument(std::string(who) + ": a histogram is attached already");
    if (b->units_added.load() != 0) throw std::invalid_argument(std::string(who) + ": reads have been added already");
    speq_device_index* d = b->dev;
    DeviceGuard g(d->device);
    const uint64_t n_rows = em->row_mult.size(), m = em->iv_lo.size();
    const uint32_t R = b->B + 1u;
    // slots: the rows by descending multiplicity of the sample, ties by row index, so that the hot rows are the ones
    // a block keeps in LDS
    std::vector<uint32_t> order(n_rows);
    for (uint64_t r = 0; r < n_rows; ++r) order[r] = (uint32_t)r;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t x, uint32_t y) { return em->row_mult[x] > em->row_mult[y]; });
    std::vector<uint32_t> slot_of_row(n_rows), slot(m);
    for (uint64_t s = 0; s < n_rows; ++s) slot_of_row[order[s]] = (uint32_t)s;
    for (uint64_t i = 0; i < m; ++i) slot[i] = slot_of_row[em->iv_row[i]];
    const size_t mb = (size_t)(n_rows * R * 8u);
    // (the handle takes the four arrays when they are filled: a failure leaves it without a histogram)
    DevPtr<uint32_t> lo = DevPtr<uint32_t>::alloc(m, who), sl = DevPtr<uint32_t>::alloc(m, who);
    DevPtr<unsigned long long> mult = DevPtr<unsigned long long>::alloc(mb / 8u, who);
    DevPtr<unsigned long long> missed = DevPtr<unsigned long long>::alloc(1, who);
    {
        SyncOnExit sync(d->stream);
        if (m) {
            HIP_OK(hipMemcpyAsync(lo.get(), em->iv_lo.data(), m * 4u, hipMemcpyHostToDevice, d->stream));
            HIP_OK(hipMemcpyAsync(sl.get(), slot.data(), m * 4u, hipMemcpyHostToDevice, d->stream));
        }
        HIP_OK(hipMemsetAsync(mult.get(), 0, std::max<size_t>(mb, 16), d->stream));
        HIP_OK(hipMemsetAsync(missed.get(), 0, 8, d->stream));
        HIP_OK(hipStreamSynchronize(d->stream));  // (the host vectors above are read until here)
    }
    b->d_em_lo = std::move(lo);
    b->d_em_slot = std::move(sl);
    b->d_em_mult = std::move(mult);
    b->d_em_missed = std::move(missed);
    b->em_rows = n_rows;
    b->em_m = (uint32_t)m;
    b->em_lds_rows = em_lds_rows(n_rows, R, b->G, is_local(b->params), b->params.k);
    b->em_slot_of_row.swap(slot_of_row);
    b->em_attached = true;
}

void finalize_em_impl(speq_bootstrap* b, uint64_t* mult, uint64_t* missed) {
    const char* who = "speq_bootstrap_finalize_em";
    if (!b) throw std::invalid_argument(std::string(who) + ": null handle");
    if (!b->em_attached) throw std::invalid_argument(std::string(who) + ": no histogram attached");
    if (!mult && b->em_rows) throw std::invalid_argument(std::string(who) + ": null output");
    speq_device_index* d = b->dev;
    DeviceGuard g(d->device);
    HIP_OK(hipDeviceSynchronize());  // the adds of every stream of the device have completed
    const uint64_t R = b->B + 1u, n_rows = b->em_rows;
    std::vector<uint64_t> hm((size_t)(n_rows * R));
    if (n_rows) HIP_OK(hipMemcpy(hm.data(), b->d_em_mult.get(), hm.size() * 8, hipMemcpyDeviceToHost));
    for (uint64_t row = 0; row < n_rows; ++row) {
        const uint64_t* cells = hm.data() + (uint64_t)b->em_slot_of_row[row] * R;
        for (uint64_t r = 0; r < R; ++r) mult[r * n_rows + row] = cells[r];
    }
    if (missed) HIP_OK(hipMemcpy(missed, b->d_em_missed.get(), 8, hipMemcpyDeviceToHost));
}

// ---- the summary (host only) ----
// The statistics of speq_bootstrap_summary over value(b, g), b = 1 .. B where used(b); estimate(g) is the sample's.
template <class Value, class Used, class Estimate>
void summarise(uint32_t replicates, uint32_t G, double level, Value&& value, Used&& used, Estimate&& estimate,
               speq_bootstrap_ci* out) {
    std::vector<double> v;
    for (uint32_t g = 0; g < G; ++g) {
        speq_bootstrap_ci ci{};
        ci.estimate = estimate(g);
        v.clear();
        for (uint32_t b = 1; b <= replicates; ++b)
            if (used(b)) v.push_back(value(b, g));
        const size_t n = v.size();
        ci.used = n;
        if (n) {
            double s = 0.0;
            for (double x : v) s += x;
            ci.mean = s / (double)n;
            if (n >= 2) {
                double q = 0.0;
                for (double x : v) q += (x - ci.mean) * (x - ci.mean);
                ci.se = std::sqrt(q / (double)(n - 1));
            }
            std::sort(v.begin(), v.end());
            const size_t t = (size_t)std::floor((double)n * (1.0 - level) / 2.0);
            ci.lo = v[t];
            ci.hi = v[n - 1 - t];
        }
        out[g] = ci;
    }
}

void check_summary_args(const char* who, uint32_t replicates, double level) {
    if (replicates < 1 || replicates > SPEQ_BOOTSTRAP_MAX_REPLICATES)
        throw std::invalid_argument(std::string(who) + ": replicates must be in [1, " +
                                    std::to_string(SPEQ_BOOTSTRAP_MAX_REPLICATES) + "]");
    if (!(level > 0.0 && level < 1.0)) throw std::invalid_argument(std::string(who) + ": level must be in (0, 1)");
}

void summary_percent_impl(const double* percent, const double* estimate, const uint8_t* used_mask, uint32_t replicates,
                          uint32_t n_groups, double level, speq_bootstrap_ci* out) {
    const char* who = "speq_bootstrap_summary_percent";
    if (!percent || !used_mask || !out) throw std::invalid_argument(std::string(who) + ": null argument");
    check_summary_args(who, replicates, level);
    const uint32_t G = n_groups;
    summarise(
        replicates, G, level, [&](uint32_t b, uint32_t g) { return percent[(size_t)b * G + g]; },
        [&](uint32_t b) { return used_mask[b] != 0; }, [&](uint32_t g) { return estimate ? estimate[g] : percent[g]; },
        out);
}

void summary_impl(const uint64_t* counts, const double* weights, uint32_t replicates, uint32_t n_groups,
                  const uint64_t* u_ref, const uint64_t* tot_ref, double unique_scale, double level,
                  speq_bootstrap_ci* out) {
    const char* who = "speq_bootstrap_summary";
    if (!counts || !u_ref || !tot_ref || !out) throw std::invalid_argument(std::string(who) + ": null argument");
    check_summary_args(who, replicates, level);
    const uint32_t G = n_groups, C = G + 2u;
    // unique_to_percent (fm_scanner.cpp:1455-1474) of row b
    auto percent = [&](uint32_t b, uint32_t g) {
        if (!((double)tot_ref[g] > 0.0)) return 0.0;
        const double ur = weights ? weights[(size_t)b * G + g] : (double)counts[(size_t)b * C + 2u + g] * unique_scale;
        const double pu = (double)u_ref[g] / (double)tot_ref[g];
        return 100.0 * ur / (double)counts[(size_t)b * C] / pu;
    };
    summarise(
        replicates, G, level, percent, [&](uint32_t b) { return counts[(size_t)b * C] != 0; },
        [&](uint32_t g) { return percent(0, g); }, out);
}

}  // namespace

static_assert(sizeof(speq_bootstrap_ci) == 48, "speq_bootstrap_ci is five doubles and a u64");

extern "C" {

int speq_bootstrap_create(speq_device_index* d, const speq_scan_params* params, uint32_t replicates, uint64_t seed,
                          speq_bootstrap** out) {
    return speq::guarded_nomem([&] { create_impl(d, params, replicates, seed, out); });
}

int speq_bootstrap_add_reads_device(speq_bootstrap* b, const uint8_t* d_seq, const uint8_t* d_qual,
                                    const uint64_t* d_offsets, uint64_t n_reads, uint64_t first_unit, void* stream) {
    return speq::guarded_nomem(
        [&] { add_device_impl(b, d_seq, d_qual, d_offsets, n_reads, first_unit, static_cast<hipStream_t>(stream)); });
}

int speq_bootstrap_add_reads(speq_bootstrap* b, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                             uint64_t n_reads, uint64_t first_unit) {
    return speq::guarded_nomem([&] { add_host_impl(b, seq, qual, offsets, n_reads, first_unit); });
}

int speq_bootstrap_finalize(speq_bootstrap* b, uint64_t* counts, double* weights) {
    return speq::guarded_nomem([&] { finalize_impl(b, counts, weights); });
}

int speq_bootstrap_info(const speq_bootstrap* b, uint32_t* replicates, uint32_t* lds_path, uint64_t* units_added) {
    return speq::guarded([&] {
        if (!b) throw std::invalid_argument("speq_bootstrap_info: null handle");
        if (replicates) *replicates = b->B;
        if (lds_path) *lds_path = b->lds_path.load();
        if (units_added) *units_added = b->units_added.load();
    });
}

void speq_bootstrap_free(speq_bootstrap* b) { delete b; }

int speq_bootstrap_attach_em(speq_bootstrap* b, const speq_em* em) {
    return speq::guarded_nomem([&] { attach_em_impl(b, em); });
}

int speq_bootstrap_em_info(const speq_bootstrap* b, uint64_t* n_rows, uint32_t* lds_rows) {
    return speq::guarded([&] {
        if (!b) throw std::invalid_argument("speq_bootstrap_em_info: null handle");
        if (!b->em_attached) throw std::invalid_argument("speq_bootstrap_em_info: no histogram attached");
        if (n_rows) *n_rows = b->em_rows;
        if (lds_rows) *lds_rows = b->em_lds_rows;
    });
}

int speq_bootstrap_finalize_em(speq_bootstrap* b, uint64_t* mult, uint64_t* missed) {
    return speq::guarded_nomem([&] { finalize_em_impl(b, mult, missed); });
}

int speq_bootstrap_summary_percent(const double* percent, const double* estimate, const uint8_t* used_mask,
                                   uint32_t replicates, uint32_t n_groups, double level, speq_bootstrap_ci* out) {
    return speq::guarded(
        [&] { summary_percent_impl(percent, estimate, used_mask, replicates, n_groups, level, out); });
}

uint32_t speq_bootstrap_weight(uint64_t seed, uint64_t unit, uint32_t replicate) {
    return replicate == 0 ? 1u : weight_of(draw(unit_key(seed, unit), replicate));
}

int speq_bootstrap_summary(const uint64_t* counts, const double* weights, uint32_t replicates, uint32_t n_groups,
                           const uint64_t* u_ref, const uint64_t* tot_ref, double unique_scale, double level,
                           speq_bootstrap_ci* out) {
    return speq::guarded(
        [&] { summary_impl(counts, weights, replicates, n_groups, u_ref, tot_ref, unique_scale, level, out); });
}

}  // extern "C"
