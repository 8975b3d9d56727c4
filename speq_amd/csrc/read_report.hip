// Per-unit report (speq_report_reads_device / speq_report_reads): for every read, or pair, the number
// of passing, single-group and multi-group windows, the group of its first single-group window and the set of groups
// its windows are unique to. A diagnostic pass beside the scan kernels: every passing window gets an exact backward
// search (search_lds), no per-k structure is used, and nothing here is on the hot path of `speq scan`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "device_index.hpp"
#include "scan_device.hpp"

namespace {

using namespace speq_dev;

constexpr uint32_t NO_GROUP = 0xFFFFFFFFu;

// Per-wave LDS: u16 prefix counts of bad positions [64 + k] | symbol codes [64 + k - 1], rounded to 16 B.
__host__ __device__ inline uint32_t report_wave_bytes(uint32_t k) { return (3u * (64u + k) + 15u) & ~15u; }

// One wave64 owns one unit (a read, or the pair 2u, 2u + 1) and walks each mate in tiles of 64 window starts. A tile
// stages the 64 + k - 1 positions under its windows: the symbol code of each and the number of bad positions (N, or
// quality <= cutoff) before it, so window j passes iff cnt[j + k] == cnt[j] (two LDS loads). Lane j then searches
// window tile + j; ballots fold the lanes' results into the unit's record and group set. No other wave touches the
// unit's rows, so lane 0 writes them with plain loads and stores (the launcher cleared the set rows).
template <bool PAIRED>
__global__ __launch_bounds__(BLOCK_THREADS) void k_read_report(const DevView I, const uint8_t* __restrict__ seq,
                                                               const uint8_t* __restrict__ qual,
                                                               const uint64_t* __restrict__ off, uint64_t n_units,
                                                               uint32_t k, uint32_t cutoff, uint32_t W,
                                                               uint4* __restrict__ reports,
                                                               uint64_t* __restrict__ sets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned char* base = lds + wave * report_wave_bytes(k);
    uint16_t* cnt = reinterpret_cast<uint16_t*>(base);
    unsigned char* sym = base + 2u * (64u + k);
    const Rsrc R = make_rsrc(I);
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t u = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; u < n_units;
         u += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        uint32_t passing = 0, unique = 0, shared = 0, first = NO_GROUP;
        uint64_t* row = sets + u * W;
        for (uint32_t m = 0; m < (PAIRED ? 2u : 1u); ++m) {
            const uint64_t r = PAIRED ? 2u * u + m : u;
            const uint64_t beg = off[r], len = off[r + 1] - beg;
            if (len < k) continue;
            const uint64_t nwin = len - k + 1u;
            for (uint64_t tile = 0; tile < nwin; tile += 64u) {
                const uint32_t span = (uint32_t)min((uint64_t)(64u + k - 1u), len - tile);  // staged positions
                uint32_t bad_before = 0;
                for (uint32_t c = 0; c < span; c += 64u) {
                    const uint32_t p = c + lane;
                    const bool valid = p < span;
                    uint32_t s = 4u;
                    bool bad = false;
                    if (valid) {
                        const uint64_t at = beg + tile + p;
                        s = ascii_sym(seq[at]);
                        const int32_t q = min(max((int32_t)qual[at] - 33, 0), 41);
                        bad = s == 4u || (uint32_t)q <= cutoff;
                    }
                    const uint64_t bal = __ballot(bad);
                    if (valid) {
                        sym[p] = (unsigned char)s;
                        cnt[p] = (uint16_t)(bad_before + (uint32_t)__popcll(bal & below));
                    }
                    bad_before += (uint32_t)__popcll(bal);
                }
                if (lane == 0) cnt[span] = (uint16_t)bad_before;
                wave_sync();
                const bool has = tile + lane < nwin;  // then lane + k <= span
                const bool pass = has && cnt[lane + k] == cnt[lane];
                int res = -1;
                if (pass) {
                    uint32_t lo, hi;
                    res = search_lds(I, R, sym + lane, k, true, lo, hi);
                }
                const uint64_t b_uni = __ballot(res >= 0);
                passing += (uint32_t)__popcll(__ballot(pass));
                unique += (uint32_t)__popcll(b_uni);
                shared += (uint32_t)__popcll(__ballot(res == -2));
                if (b_uni != 0ull) {
                    if (first == NO_GROUP) first = (uint32_t)__shfl(res, __builtin_ctzll(b_uni));
                    uint64_t rest = b_uni;  // wave-uniform: one round per distinct group of the tile
                    while (rest != 0ull) {
                        const int g = __shfl(res, __builtin_ctzll(rest));
                        rest &= ~__ballot(res == g);
                        if (lane == 0 && (uint32_t)g < I.G) row[(uint32_t)g >> 6] |= 1ull << ((uint32_t)g & 63u);
                    }
                }
                wave_sync();  // the next tile restages this wave's region
            }
        }
        if (lane == 0) reports[u] = make_uint4(passing, unique, shared, first);
    }
}

void check_params(const char* who, const speq_device_index* d, const speq_scan_params* p, uint64_t n_reads) {
    if (!p) throw std::invalid_argument(std::string(who) + ": null params");
    if (p->k < 1 || p->k > SPEQ_REPORT_MAX_K)
        throw std::invalid_argument(std::string(who) + ": k must be in [1, 1024]");
    if (p->paired && (n_reads & 1))
        throw std::invalid_argument(std::string(who) + ": paired report needs an even record count");
    if (!d) throw std::invalid_argument(std::string(who) + ": null device index");
}

void report_device_impl(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_offsets,
                        uint64_t n_reads, const speq_scan_params* p, speq_read_report* d_reports, uint64_t* d_sets,
                        hipStream_t st) {
    check_params("speq_report_reads_device", d, p, n_reads);
    const uint64_t n_units = p->paired ? n_reads / 2 : n_reads;
    if (n_units == 0) return;
    if (!d_seq || !d_qual || !d_offsets || !d_reports || !d_sets)
        throw std::invalid_argument("speq_report_reads_device: null buffer");
    if ((reinterpret_cast<uintptr_t>(d_reports) & 15u) || (reinterpret_cast<uintptr_t>(d_sets) & 7u))
        throw std::invalid_argument("speq_report_reads_device: reports must be 16-byte and sets 8-byte aligned");
    DeviceGuard g(d->device);
    const uint32_t W = (uint32_t)SPEQ_SET_WORDS(d->G);
    HIP_OK(hipMemsetAsync(d_sets, 0, n_units * W * sizeof(uint64_t), st));
    const DevView v = speq::search_view(d, p->k);
    const size_t lds = (size_t)WAVES_PER_BLOCK * report_wave_bytes(p->k);  // 13 KiB at k = 1024
    const uint64_t blocks = std::min<uint64_t>((n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384u);
    uint4* rep = reinterpret_cast<uint4*>(d_reports);
    if (p->paired)
        hipLaunchKernelGGL(k_read_report<true>, dim3((uint32_t)blocks), dim3(BLOCK_THREADS), lds, st, v, d_seq, d_qual,
                           d_offsets, n_units, p->k, p->phred_cutoff, W, rep, d_sets);
    else
        hipLaunchKernelGGL(k_read_report<false>, dim3((uint32_t)blocks), dim3(BLOCK_THREADS), lds, st, v, d_seq, d_qual,
                           d_offsets, n_units, p->k, p->phred_cutoff, W, rep, d_sets);
    HIP_OK(hipGetLastError());
}

struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 16))); }
    ~DevBuf() { (void)hipFree(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// Batches of whole units: at most BATCH_RECORDS records and (a single longer unit aside) BATCH_BYTES bases each.
constexpr uint64_t BATCH_RECORDS = 1ull << 20, BATCH_BYTES = 256ull << 20;

void report_host_impl(speq_device_index* d, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                      uint64_t n_reads, const speq_scan_params* p, speq_read_report* reports, uint64_t* sets) {
    check_params("speq_report_reads", d, p, n_reads);
    if (n_reads == 0) return;
    if (!offsets || !reports || !sets) throw std::invalid_argument("speq_report_reads: null argument");
    for (uint64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i]) throw std::invalid_argument("speq_report_reads: offsets must be non-decreasing");
    if (offsets[n_reads] > offsets[0] && (!seq || !qual)) throw std::invalid_argument("speq_report_reads: null read buffer");
    const uint32_t per = p->paired ? 2u : 1u;
    const uint32_t W = (uint32_t)SPEQ_SET_WORDS(d->G);
    DeviceGuard g(d->device);
    // one report at a time per process: the batches go through the replica's stream and wait for it
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    std::vector<uint64_t> rel;
    for (uint64_t r0 = 0; r0 < n_reads;) {
        uint64_t r1 = r0 + per;
        while (r1 < n_reads && r1 + per - r0 <= BATCH_RECORDS && offsets[r1 + per] - offsets[r0] <= BATCH_BYTES) r1 += per;
        const uint64_t n = r1 - r0, units = n / per, bytes = offsets[r1] - offsets[r0];
        rel.resize(n + 1);
        for (uint64_t i = 0; i <= n; ++i) rel[i] = offsets[r0 + i] - offsets[r0];
        DevBuf ds(bytes), dq(bytes), dof((n + 1) * 8), drep(units * sizeof(speq_read_report)), dset(units * W * 8);
        if (bytes) {
            HIP_OK(hipMemcpyAsync(ds.p, seq + offsets[r0], bytes, hipMemcpyHostToDevice, d->stream));
            HIP_OK(hipMemcpyAsync(dq.p, qual + offsets[r0], bytes, hipMemcpyHostToDevice, d->stream));
        }
        HIP_OK(hipMemcpyAsync(dof.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, d->stream));
        report_device_impl(d, static_cast<const uint8_t*>(ds.p), static_cast<const uint8_t*>(dq.p),
                           static_cast<const uint64_t*>(dof.p), n, p, static_cast<speq_read_report*>(drep.p),
                           static_cast<uint64_t*>(dset.p), d->stream);
        const uint64_t u0 = r0 / per;
        HIP_OK(hipMemcpyAsync(reports + u0, drep.p, units * sizeof(speq_read_report), hipMemcpyDeviceToHost, d->stream));
        HIP_OK(hipMemcpyAsync(sets + u0 * W, dset.p, units * W * 8, hipMemcpyDeviceToHost, d->stream));
        HIP_OK(hipStreamSynchronize(d->stream));
        r0 = r1;
    }
}

}  // namespace

static_assert(sizeof(speq_read_report) == 16, "speq_read_report is one 16-byte store");

extern "C" {

int speq_report_reads_device(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual,
                             const uint64_t* d_offsets, uint64_t n_reads, const speq_scan_params* params,
                             speq_read_report* d_reports, uint64_t* d_sets, void* stream) {
    return speq::guarded([&] {
        report_device_impl(d, d_seq, d_qual, d_offsets, n_reads, params, d_reports, d_sets,
                           static_cast<hipStream_t>(stream));
    });
}

int speq_report_reads(speq_device_index* d, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                      uint64_t n_reads, const speq_scan_params* params, speq_read_report* reports, uint64_t* sets) {
    return speq::guarded([&] { report_host_impl(d, seq, qual, offsets, n_reads, params, reports, sets); });
}

}  // extern "C"
