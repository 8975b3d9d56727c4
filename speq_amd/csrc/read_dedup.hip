// Duplicate reads (speq_dedup_*): every unit (a read, or the pair 2u, 2u + 1) gets a 128-bit fingerprint
// of its dna5-converted bases; units of equal fingerprint are duplicates, and the one of lowest index is kept. The
// records of the others get their qualities overwritten with '!' (Phred 0) in the staged copy of a batch, so that the
// unchanged scan kernels count none of their windows: a window passes only if every quality is above an unsigned
// cutoff. Two distinct sequences get the same fingerprint with probability about 2^-128 per pair. A pass beside the
// scan kernels: a fingerprint kernel (each base read once, no search), two radix sorts and a mark kernel, and a mask
// kernel. Nothing here runs in a `speq scan` without --dedup.
#include <hip/hip_runtime.h>

#include <cstring>  // rocprim/iterator/texture_cache_iterator.hpp uses ::memset

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "em.hpp"
#include "window_pass.hpp"

namespace {

// Storage grows in chunks of CHUNK units, each allocated when an add first reaches it and never moved, so an add waits
// for nothing but (once per chunk) the zeroing of the chunk's `seen` words. One allocation per chunk:
// u64 F0[CHUNK] | u64 F1[CHUNK] | u32 seen[CHUNK] (how often the unit was added): 20 bytes per unit.
constexpr uint32_t CHUNK_LOG = 16;
constexpr uint64_t CHUNK = 1ull << CHUNK_LOG;
constexpr uint64_t CHUNK_BYTES = CHUNK * 20u;
constexpr uint64_t MAX_UNITS = 0xFFFFFFFFull;  // unit indices are below 2^32 - 1

}  // namespace

struct speq_dedup {
    speq_device_index* dev = nullptr;
    bool paired = false;
    std::mutex mu;                      // everything below
    std::vector<speq_dev::DevPtr<unsigned char>> chunks;  // chunk c holds the units c * CHUNK ..; null: not reached yet
    hipStream_t zero_stream = nullptr;  // the zeroing of a new chunk's seen words, waited for before the chunk is used
    uint64_t units_added = 0, end_unit = 0;  // units of every add; one past the highest unit added
    bool finalized = false;             // a finalize succeeded and no add came after it
    uint64_t n = 0;                     // units of that finalize
    speq_dev::DevPtr<uint32_t> d_rep;   // [rep_cap]: rep[u] of that finalize
    uint64_t rep_cap = 0;
    ~speq_dedup() {
        if (zero_stream) (void)hipStreamDestroy(zero_stream);
    }
};

namespace {

using namespace speq_dev;

// ---- the fingerprint (integer only; tests/dedup_model.py restates it) ----
constexpr uint64_t GAMMA = 0x9e3779b97f4a7c15ull;
constexpr uint64_t S0 = 0x243f6a8885a308d3ull, S1 = 0x13198a2e03707344ull;
// splitmix64's finaliser
__host__ __device__ inline uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// the scan's dna5 conversion: the device uses ascii_sym itself, the host its definition written out
__host__ __device__ inline uint32_t base_code(uint32_t ch) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ascii_sym(ch);
#else
    switch (ch | 0x20u) {
        case 'a': return 0u;
        case 'c': return 1u;
        case 'g': return 2u;
        case 't':
        case 'u': return 3u;
        default: return 4u;
    }
#endif
}
// adds base code c at position i of mate m to both streams' sums
__host__ __device__ inline void add_term(uint32_t c, uint64_t i, uint32_t m, uint64_t& f0, uint64_t& f1) {
    const uint64_t x = GAMMA * (1ull + c + 5ull * i + ((uint64_t)m << 40));
    f0 += mix(S0 + x);
    f1 += mix(S1 + x);
}

__device__ __forceinline__ const uint64_t* chunk_f0(const unsigned char* const* tbl, uint32_t u) {
    return reinterpret_cast<const uint64_t*>(tbl[u >> CHUNK_LOG]) + (u & (CHUNK - 1u));
}
__device__ __forceinline__ uint64_t fp0(const unsigned char* const* tbl, uint32_t u) { return *chunk_f0(tbl, u); }
__device__ __forceinline__ uint64_t fp1(const unsigned char* const* tbl, uint32_t u) { return chunk_f0(tbl, u)[CHUNK]; }
__device__ __forceinline__ uint32_t seen_of(const unsigned char* const* tbl, uint32_t u) {
    return reinterpret_cast<const uint32_t*>(tbl[u >> CHUNK_LOG] + 16u * CHUNK)[u & (CHUNK - 1u)];
}

// One wave64 owns one unit: lanes take consecutive bases of each mate (byte loads: a read starts at any byte offset),
// every lane sums its bases' terms of both streams, the wave adds the 64 partial sums, and lane 0 stores (F0, F1) and
// counts the add in seen. off points at the offsets of the launch's first record, f0 / f1 / seen at its first unit.
template <bool PAIRED>
__global__ __launch_bounds__(BLOCK_THREADS) void k_dedup_fingerprint(const uint8_t* __restrict__ seq,
                                                                     const uint64_t* __restrict__ off, uint32_t n_units,
                                                                     uint64_t* __restrict__ f0, uint64_t* __restrict__ f1,
                                                                     uint32_t* __restrict__ seen) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t u = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; u < n_units;
         u += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        uint64_t a0 = 0, a1 = 0;
        for (uint32_t m = 0; m < (PAIRED ? 2u : 1u); ++m) {
            const uint64_t r = PAIRED ? 2u * u + m : u;
            const uint64_t beg = off[r], len = off[r + 1] - beg;
            const uint8_t* s = seq + beg;
#pragma unroll 4
            for (uint64_t i = lane; i < len; i += 64u) add_term(base_code(s[i]), i, m, a0, a1);
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane == 0u) {
            f0[u] = a0;
            f1[u] = a1;
            atomicAdd(&seen[u], 1u);
        }
    }
}

// First sort key and the identity permutation; *bad counts the units not added exactly once.
__global__ void k_dedup_keys1(const unsigned char* const* __restrict__ tbl, uint32_t n, uint64_t* __restrict__ keys,
                              uint32_t* __restrict__ vals, unsigned long long* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = fp1(tbl, i);
    vals[i] = i;
    if (seen_of(tbl, i) != 1u) atomicAdd(bad, 1ull);
}

// Second sort key, of the units in the order the first sort left them
__global__ void k_dedup_keys2(const unsigned char* const* __restrict__ tbl, uint32_t n,
                              const uint32_t* __restrict__ vals, uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = fp0(tbl, vals[i]);
}

// head value for the max-scan: i where a class starts (the (F0, F1) pair differs from the left neighbour's), else 0
__global__ void k_dedup_heads(const unsigned char* const* __restrict__ tbl, uint32_t n,
                              const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                              uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool h = i == 0u || keys[i] != keys[i - 1u] || fp1(tbl, vals[i]) != fp1(tbl, vals[i - 1u]);
    head[i] = h ? i : 0u;
}

// head[i] now holds the position of i's class head (inclusive max-scan); equal fingerprints stand in ascending unit
// order (both sorts are stable and started from the identity), so the head's unit is the class's lowest. The last
// position of a class knows its size: classes, the largest size and the size bins are tallied per block in LDS and
// added to stats (u64: [1] distinct, [2] max_multiplicity, [4 + j] mult_hist[j]) once per block, integer adds only.
__global__ __launch_bounds__(256) void k_dedup_mark(uint32_t n, const uint32_t* __restrict__ vals,
                                                    const uint32_t* __restrict__ head, uint32_t* __restrict__ rep,
                                                    unsigned long long* __restrict__ stats) {
    __shared__ uint32_t tally[10];  // [0] classes, [1] largest size, [2 + j] bins
    if (threadIdx.x < 10u) tally[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t h = head[i];
        rep[vals[i]] = vals[h];
        if (i + 1u == n || head[i + 1u] == i + 1u) {
            const uint32_t size = i - h + 1u;
            atomicAdd(&tally[0], 1u);
            atomicMax(&tally[1], size);
            atomicAdd(&tally[2u + min(size, (uint32_t)8u) - 1u], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 10u && tally[threadIdx.x] != 0u) {
        const uint32_t t = threadIdx.x;
        if (t == 0u) atomicAdd(&stats[1], (unsigned long long)tally[0]);
        else if (t == 1u) atomicMax(&stats[2], (unsigned long long)tally[1]);
        else atomicAdd(&stats[4u + t - 2u], (unsigned long long)tally[t]);
    }
}

// One wave64 per record: the record r of a unit that is not its class's representative gets '!' over its quality
// bytes, and nothing else is written. rep points at rep[first_unit].
__global__ __launch_bounds__(BLOCK_THREADS) void k_dedup_mask(uint8_t* __restrict__ qual,
                                                              const uint64_t* __restrict__ off, uint64_t n_reads,
                                                              uint32_t per, uint32_t first_unit,
                                                              const uint32_t* __restrict__ rep) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; r < n_reads;
         r += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t u = r / per;
        if (rep[u] == first_unit + (uint32_t)u) continue;  // kept
        const uint64_t beg = off[r], end = off[r + 1];
        for (uint64_t i = beg + lane; i < end; i += 64u) qual[i] = (uint8_t)'!';
    }
}

inline uint32_t grid1d(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }
// blocks of four waves, one wave per item, striding past the cap
inline uint32_t wave_grid(uint64_t items) {
    return (uint32_t)std::min<uint64_t>((items + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 65536u);
}

void create_impl(speq_device_index* d, uint32_t paired, speq_dedup** out) {
    const char* who = "speq_dedup_create";
    if (!d) throw std::invalid_argument(std::string(who) + ": null device index");
    if (!out) throw std::invalid_argument(std::string(who) + ": null output");
    DeviceGuard g(d->device);
    auto h = std::make_unique<speq_dedup>();
    h->dev = d;
    h->paired = paired != 0;
    HIP_OK(hipStreamCreateWithFlags(&h->zero_stream, hipStreamNonBlocking));
    *out = h.release();
}

// the chunk of unit u, allocated and its seen words zeroed on first use (h->mu held)
unsigned char* chunk_for(speq_dedup* h, uint64_t u, const char* who) {
    const size_t c = (size_t)(u >> CHUNK_LOG);
    if (h->chunks.size() <= c) h->chunks.resize(c + 1);
    if (!h->chunks[c]) {
        DevPtr<unsigned char> p = DevPtr<unsigned char>::alloc(CHUNK_BYTES, who);
        SyncOnExit sync(h->zero_stream);
        // the adds come on the callers' streams: the zeros are in place before any of them can reach the chunk
        HIP_OK(hipMemsetAsync(p.get() + 16u * CHUNK, 0, 4u * CHUNK, h->zero_stream));
        HIP_OK(hipStreamSynchronize(h->zero_stream));
        h->chunks[c] = std::move(p);
    }
    return h->chunks[c].get();
}

void check_units(const char* who, const speq_dedup* h, uint64_t n_reads, uint64_t first_unit) {
    if (h->paired && (n_reads & 1))
        throw std::invalid_argument(std::string(who) + ": a paired handle needs an even record count");
    const uint64_t n_units = h->paired ? n_reads / 2 : n_reads;
    if (first_unit > MAX_UNITS || n_units > MAX_UNITS - first_unit)
        throw std::invalid_argument(std::string(who) + ": unit indices must stay below 2^32 - 1");
}

void add_device_impl(speq_dedup* h, const uint8_t* d_seq, const uint64_t* d_offsets, uint64_t n_reads,
                     uint64_t first_unit, hipStream_t st) {
    const char* who = "speq_dedup_add_reads_device";
    if (n_reads > 0 && (!d_seq || !d_offsets)) throw std::invalid_argument(std::string(who) + ": null buffer");
    if (!h) throw std::invalid_argument(std::string(who) + ": null handle");
    check_units(who, h, n_reads, first_unit);
    const uint32_t per = h->paired ? 2u : 1u;
    const uint64_t n_units = n_reads / per;
    if (n_units == 0) return;
    DeviceGuard g(h->dev->device);
    std::lock_guard<std::mutex> lk(h->mu);
    h->finalized = false;
    // one launch per chunk the units reach
    for (uint64_t u0 = first_unit, end = first_unit + n_units; u0 < end;) {
        const uint64_t u1 = std::min(end, ((u0 >> CHUNK_LOG) + 1u) << CHUNK_LOG), slot = u0 & (CHUNK - 1u);
        unsigned char* c = chunk_for(h, u0, who);
        uint64_t* f0 = reinterpret_cast<uint64_t*>(c) + slot;
        uint32_t* seen = reinterpret_cast<uint32_t*>(c + 16u * CHUNK) + slot;
        const uint64_t* off = d_offsets + (u0 - first_unit) * per;
        const uint32_t n = (uint32_t)(u1 - u0);
        if (h->paired)
            hipLaunchKernelGGL(k_dedup_fingerprint<true>, dim3(wave_grid(n)), dim3(BLOCK_THREADS), 0, st, d_seq, off, n,
                               f0, f0 + CHUNK, seen);
        else
            hipLaunchKernelGGL(k_dedup_fingerprint<false>, dim3(wave_grid(n)), dim3(BLOCK_THREADS), 0, st, d_seq, off, n,
                               f0, f0 + CHUNK, seen);
        HIP_OK(hipGetLastError());
        h->units_added += n;
        h->end_unit = std::max(h->end_unit, u1);
        u0 = u1;
    }
}

void add_host_impl(speq_dedup* h, const uint8_t* seq, const uint64_t* offsets, uint64_t n_reads, uint64_t first_unit) {
    const char* who = "speq_dedup_add_reads";
    // (the handle last: every check of the arrays is made before anything of the device is touched)
    if (n_reads > 0 && !offsets) throw std::invalid_argument(std::string(who) + ": null offsets");
    speq::check_host_reads(who, seq, seq, offsets, n_reads);
    if (!h) throw std::invalid_argument(std::string(who) + ": null handle");
    check_units(who, h, n_reads, first_unit);
    if (n_reads == 0) return;
    speq_device_index* d = h->dev;
    DeviceGuard g(d->device);
    const uint32_t per = h->paired ? 2u : 1u;
    // the shared staging copies a quality array with the bases: the bases stand in for it, the add reads neither
    for_staged_batches(who, d, seq, seq, offsets, n_reads, per,
                       [&](const uint8_t* d_seq, const uint8_t*, const uint64_t* d_off, uint64_t r0, uint64_t n) {
                           add_device_impl(h, d_seq, d_off, n, first_unit + r0 / per, d->stream);
                       });
}

void finalize_impl(speq_dedup* h, speq_dedup_stats* out) {
    const char* who = "speq_dedup_finalize";
    if (!h) throw std::invalid_argument(std::string(who) + ": null handle");
    if (!out) throw std::invalid_argument(std::string(who) + ": null output");
    speq_device_index* d = h->dev;
    DeviceGuard g(d->device);
    HIP_OK(hipDeviceSynchronize());  // the adds of every stream of the device have completed
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t N = h->end_unit;
    const char* not_once = ": the units added so far are not 0 .. N - 1, each once";
    if (h->units_added != N) throw std::invalid_argument(std::string(who) + not_once);
    const size_t n_chunks = (size_t)((N + CHUNK - 1) >> CHUNK_LOG);
    for (size_t c = 0; c < n_chunks; ++c)
        if (!h->chunks[c]) throw std::invalid_argument(std::string(who) + not_once);
    speq_dedup_stats stats{};
    if (N != 0) {
        const uint32_t n = (uint32_t)N;
        hipStream_t st = d->stream;
        if (h->rep_cap < N) {
            h->d_rep.reset();  // first, so that the two are never alive together
            h->rep_cap = 0;
            h->d_rep = DevPtr<uint32_t>::alloc(N, who);
            h->rep_cap = N;
        }
        std::vector<const unsigned char*> table(n_chunks);  // the chunks' addresses, for the kernels
        for (size_t c = 0; c < n_chunks; ++c) table[c] = h->chunks[c].get();
        const DevPtr<const unsigned char*> tbl = DevPtr<const unsigned char*>::alloc(n_chunks, who);
        const DevPtr<uint64_t> k0 = DevPtr<uint64_t>::alloc(N, who), k1 = DevPtr<uint64_t>::alloc(N, who);
        const DevPtr<uint32_t> v0 = DevPtr<uint32_t>::alloc(N, who), v1 = DevPtr<uint32_t>::alloc(N, who),
                               head = DevPtr<uint32_t>::alloc(N, who);
        const DevPtr<unsigned long long> dst = DevPtr<unsigned long long>::alloc(12, who);
        DevTemp tmp;  // rocprim's temporary storage
        SyncOnExit sync(st);
        const unsigned char* const* T = tbl.get();
        unsigned long long* d_stats = dst.get();  // [3] counts the units not added once
        HIP_OK(hipMemcpyAsync(tbl.get(), table.data(), n_chunks * sizeof(void*), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(d_stats, 0, 12u * 8u, st));
        hipLaunchKernelGGL(k_dedup_keys1, dim3(grid1d(N)), dim3(256), 0, st, T, n, k0.get(), v0.get(),
                           d_stats + 3);
        HIP_OK(hipGetLastError());
        unsigned long long bad = 0;
        HIP_OK(hipMemcpyAsync(&bad, d_stats + 3, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (bad != 0) throw std::invalid_argument(std::string(who) + not_once);
        // two stable sorts from the identity, by F1 and then by F0: equal fingerprints end up in ascending unit order
        rocprim::double_buffer<uint64_t> kb(k0.get(), k1.get());
        rocprim::double_buffer<uint32_t> vb(v0.get(), v1.get());
        size_t need = 0;
        HIP_OK(rocprim::radix_sort_pairs(nullptr, need, kb, vb, N, 0, 64, st));
        HIP_OK(rocprim::radix_sort_pairs(tmp.need(need, who), need, kb, vb, N, 0, 64, st));
        hipLaunchKernelGGL(k_dedup_keys2, dim3(grid1d(N)), dim3(256), 0, st, T, n, vb.current(), kb.current());
        HIP_OK(hipGetLastError());
        HIP_OK(rocprim::radix_sort_pairs(nullptr, need, kb, vb, N, 0, 64, st));
        HIP_OK(rocprim::radix_sort_pairs(tmp.need(need, who), need, kb, vb, N, 0, 64, st));
        uint32_t* hd = head.get();
        hipLaunchKernelGGL(k_dedup_heads, dim3(grid1d(N)), dim3(256), 0, st, T, n, kb.current(), vb.current(), hd);
        HIP_OK(hipGetLastError());
        HIP_OK(rocprim::inclusive_scan(nullptr, need, hd, hd, N, rocprim::maximum<uint32_t>(), st));
        HIP_OK(rocprim::inclusive_scan(tmp.need(need, who), need, hd, hd, N, rocprim::maximum<uint32_t>(), st));
        hipLaunchKernelGGL(k_dedup_mark, dim3(grid1d(N)), dim3(256), 0, st, n, vb.current(), hd, h->d_rep.get(), d_stats);
        HIP_OK(hipGetLastError());
        unsigned long long hs[12];
        HIP_OK(hipMemcpyAsync(hs, d_stats, sizeof hs, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        stats.distinct = hs[1];
        stats.max_multiplicity = hs[2];
        for (int j = 0; j < SPEQ_DEDUP_BINS; ++j) stats.mult_hist[j] = hs[4 + j];
    }
    stats.units = N;
    stats.reserved = 0;
    h->n = N;
    h->finalized = true;
    *out = stats;
}

// a finalize with no add after it, and the units first_unit .. first_unit + n_units - 1 inside it (h->mu held)
void check_range(const char* who, const speq_dedup* h, uint64_t first_unit, uint64_t n_units) {
    if (!h->finalized) throw std::invalid_argument(std::string(who) + ": needs a finalize with no add after it");
    if (first_unit > h->n || n_units > h->n - first_unit)
        throw std::invalid_argument(std::string(who) + ": units outside the finalized 0 .. N - 1");
}

void representatives_impl(speq_dedup* h, uint64_t first_unit, uint64_t n_units, uint32_t* rep) {
    const char* who = "speq_dedup_representatives";
    if (!h) throw std::invalid_argument(std::string(who) + ": null handle");
    if (!rep && n_units) throw std::invalid_argument(std::string(who) + ": null output");
    DeviceGuard g(h->dev->device);
    std::lock_guard<std::mutex> lk(h->mu);
    check_range(who, h, first_unit, n_units);
    if (n_units) HIP_OK(hipMemcpy(rep, h->d_rep.get() + first_unit, n_units * 4u, hipMemcpyDeviceToHost));
}

void mask_device_impl(speq_dedup* h, uint8_t* d_qual, const uint64_t* d_offsets, uint64_t n_reads, uint64_t first_unit,
                      hipStream_t st) {
    const char* who = "speq_dedup_mask_device";
    if (n_reads > 0 && (!d_qual || !d_offsets)) throw std::invalid_argument(std::string(who) + ": null buffer");
    if (!h) throw std::invalid_argument(std::string(who) + ": null handle");
    check_units(who, h, n_reads, first_unit);
    const uint32_t per = h->paired ? 2u : 1u;
    DeviceGuard g(h->dev->device);
    std::lock_guard<std::mutex> lk(h->mu);
    check_range(who, h, first_unit, n_reads / per);
    if (n_reads == 0) return;
    hipLaunchKernelGGL(k_dedup_mask, dim3(wave_grid(n_reads)), dim3(BLOCK_THREADS), 0, st, d_qual, d_offsets, n_reads,
                       per, (uint32_t)first_unit, h->d_rep.get() + first_unit);
    HIP_OK(hipGetLastError());
}

void check_rc(int rc) {
    if (rc == SPEQ_OK) return;
    if (rc == SPEQ_E_ARG) throw std::invalid_argument(speq_last_error());
    throw speq::DeviceError(speq_last_error());
}

void scan_reads_impl(speq_dedup* h, speq_em* em, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                     uint64_t n_reads, uint64_t first_unit, const speq_scan_params* p, uint64_t* counts,
                     double* weights) {
    const char* who = "speq_dedup_scan_reads";
    if (!p) throw std::invalid_argument(std::string(who) + ": null params");
    if (p->paired && (n_reads & 1)) throw std::invalid_argument(std::string(who) + ": a paired scan needs an even record count");
    if (!counts) throw std::invalid_argument(std::string(who) + ": null output");
    const bool local = p->mode == SPEQ_MODE_LOCAL;
    if (local && !weights) throw std::invalid_argument(std::string(who) + ": local mode needs weights");
    if (n_reads > 0 && !offsets) throw std::invalid_argument(std::string(who) + ": null offsets");
    speq::check_host_reads(who, seq, qual, offsets, n_reads);
    if (!h) throw std::invalid_argument(std::string(who) + ": null handle");
    if ((p->paired != 0) != h->paired) throw std::invalid_argument(std::string(who) + ": params->paired differs from the handle's");
    if (em && em->dev != h->dev) throw std::invalid_argument(std::string(who) + ": the histogram is of another replica");
    check_units(who, h, n_reads, first_unit);
    const uint32_t per = h->paired ? 2u : 1u;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        check_range(who, h, first_unit, n_reads / per);
    }
    if (n_reads == 0) return;
    speq_device_index* d = h->dev;
    DeviceGuard g(d->device);
    const uint32_t G = d->G;
    const DevPtr<uint64_t> dc = DevPtr<uint64_t>::alloc(G + 2u, who);
    const DevPtr<double> dw = DevPtr<double>::alloc(G, who);
    SyncOnExit sync(d->stream);
    uint64_t* d_counts = dc.get();
    double* d_weights = local ? dw.get() : nullptr;
    HIP_OK(hipMemsetAsync(dc.get(), 0, (G + 2u) * 8u, d->stream));
    HIP_OK(hipMemsetAsync(dw.get(), 0, std::max<size_t>(G * 8u, 16), d->stream));
    // the staged qualities are this call's own copy: the mask goes over them, the caller's arrays are only read
    for_staged_batches(who, d, seq, qual, offsets, n_reads, per,
                       [&](const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint64_t r0, uint64_t n) {
                           mask_device_impl(h, const_cast<uint8_t*>(d_qual), d_off, n, first_unit + r0 / per, d->stream);
                           check_rc(em ? speq_em_scan_reads_device(em, d_seq, d_qual, d_off, n, p, d_counts, d_weights,
                                                                   d->stream)
                                       : speq_scan_reads_device(d, d_seq, d_qual, d_off, n, p, d_counts, d_weights,
                                                                d->stream));
                       });
    std::vector<uint64_t> hc(G + 2u);
    HIP_OK(hipMemcpyAsync(hc.data(), dc.get(), hc.size() * 8u, hipMemcpyDeviceToHost, d->stream));
    std::vector<double> hw(local ? G : 0u);
    if (local && G) HIP_OK(hipMemcpyAsync(hw.data(), dw.get(), G * 8u, hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipStreamSynchronize(d->stream));
    for (uint32_t i = 0; i < G + 2u; ++i) counts[i] += hc[i];
    for (uint32_t i = 0; i < (uint32_t)hw.size(); ++i) weights[i] += hw[i];
}

}  // namespace

static_assert(sizeof(speq_dedup_stats) == 96, "speq_dedup_stats is twelve u64");

extern "C" {

int speq_dedup_create(speq_device_index* d, uint32_t paired, speq_dedup** out) {
    return speq::guarded_nomem([&] { create_impl(d, paired, out); });
}

int speq_dedup_add_reads_device(speq_dedup* h, const uint8_t* d_seq, const uint64_t* d_offsets, uint64_t n_reads,
                                uint64_t first_unit, void* stream) {
    return speq::guarded_nomem([&] { add_device_impl(h, d_seq, d_offsets, n_reads, first_unit, static_cast<hipStream_t>(stream)); });
}

int speq_dedup_add_reads(speq_dedup* h, const uint8_t* seq, const uint64_t* offsets, uint64_t n_reads,
                         uint64_t first_unit) {
    return speq::guarded_nomem([&] { add_host_impl(h, seq, offsets, n_reads, first_unit); });
}

int speq_dedup_finalize(speq_dedup* h, speq_dedup_stats* out) {
    return speq::guarded_nomem([&] { finalize_impl(h, out); });
}

int speq_dedup_representatives(speq_dedup* h, uint64_t first_unit, uint64_t n_units, uint32_t* rep) {
    return speq::guarded([&] { representatives_impl(h, first_unit, n_units, rep); });
}

int speq_dedup_mask_device(speq_dedup* h, uint8_t* d_qual, const uint64_t* d_offsets, uint64_t n_reads,
                           uint64_t first_unit, void* stream) {
    return speq::guarded(
        [&] { mask_device_impl(h, d_qual, d_offsets, n_reads, first_unit, static_cast<hipStream_t>(stream)); });
}

int speq_dedup_scan_reads(speq_dedup* h, speq_em* em, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                          uint64_t n_reads, uint64_t first_unit, const speq_scan_params* params, uint64_t* counts,
                          double* weights) {
    return speq::guarded_nomem([&] { scan_reads_impl(h, em, seq, qual, offsets, n_reads, first_unit, params, counts, weights); });
}

void speq_dedup_free(speq_dedup* h) { delete h; }

void speq_dedup_fingerprint(const uint8_t* seq1, uint64_t len1, const uint8_t* seq2, uint64_t len2, uint64_t out[2]) {
    uint64_t f0 = 0, f1 = 0;
    for (uint64_t i = 0; seq1 && i < len1; ++i) add_term(base_code(seq1[i]), i, 0u, f0, f1);
    for (uint64_t i = 0; seq2 && i < len2; ++i) add_term(base_code(seq2[i]), i, 1u, f0, f1);
    if (out) {
        out[0] = f0;
        out[1] = f1;
    }
}

}  // extern "C"
